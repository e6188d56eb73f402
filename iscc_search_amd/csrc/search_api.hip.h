// search_api.hip.h -- search_locked (every host-result search ends there: the steps of a LockedBatch), the speculation steps it shares
// with search_many, the combining queue of isccsearch_search, search_many, search_within and the document-frequency calls.
// Needs Batch, ResultBlock, record_hint and the query checks of isccsearch.hip, get_table of store.hip.h.
extern "C" {
static_assert(isksp::MAX_QUERY_SIMPRINTS == ISCCSEARCH_MAX_SCORED_SIMPRINTS, "header and kernels disagree");
// The simprint entry points: where a search leaves its lists for the scoring kernels instead of handing them to the host, what it
// queues behind every batch's select, and what it keeps of the pinned block after the batch's synchronisation
struct ScoreSink {
    SimprintScratch& sp;        // sized for the search by the caller (for_search / for_exact_search)
    int h_max = -1;
    uint32_t dup_limit = 0;
    uint32_t entries = 0;       // best (asset, query) entries appended so far -- known after each batch's synchronisation
    uint32_t max_count = 0;     // longest neighbour list
    bool unknown_any = false;   // some query's own document frequency could not be read off its list
    bool exact = false;         // isccsearch_simprint_exact: the lists are collision lists; only their lengths are kept per batch (no marking)
    uint32_t nd = 0, ng = 0;    // ... of nd distinct lookups for ng simprints as given (sp.d_of_g)
    bool prepared = false;      // ... whose hits / offsets were prepared behind the search: `entries` is known
    uint32_t* q_count = nullptr;    // when set: [nq] length of every query's neighbour list (capped at k)

    // (exact) ONE batch holds every lookup: hits / offsets are prepared behind its select, so that the number of entries arrives with
    // the batch's own synchronisation
    bool holds_every_lookup(uint32_t pos, uint32_t m) const { return exact && pos == 0 && m == nd; }
    // where the records of queries pos .. and their segment rows (nullptr: not wanted) go
    isk::Record* records(uint32_t pos, uint32_t k) const { return sp.rec.p + (size_t)pos * k; }
    uint32_t* rows(uint32_t pos, uint32_t k) const { return exact ? nullptr : sp.rows.p + (size_t)pos * k; }
    // behind the select of queries [pos, pos + m), whose lists are final on the device (or will be redone and this queued again): mark
    // the best chunk of every (asset, query) and append them to the request's entry list -- or keep the collision lists' lengths;
    // `d_info` travels to the host with the batch's block
    hipError_t queue_behind_select(uint32_t pos, uint32_t m, uint32_t k, const uint32_t* d_cnt, uint32_t* d_info, hipStream_t stream) const;
    // after the synchronisation: the info words and the lists' lengths of the pinned block
    void take(uint32_t pos, uint32_t m, uint32_t k, const uint32_t* p_cnt, const uint32_t* p_info);
};      // (both are defined beside the scoring calls, simprint_api.hip.h)

// What a search_locked call wants back -- ONE of:
//   lists         keys / hamming / prefix_bits [nq][k] and count [nq] in the caller's arrays
//   doc_freq      only the number of distinct assets per result list (doc frequency), and the lists' lengths when `collisions` is given
//   to_sink       (one-segment Hamming tables) records and rows stay in the sink's device buffers, every batch is followed by the marking /
//                 compaction kernels of simprint_score.hip, and only {counts | flags | k-th distances | info} reach the host
struct SearchOut {
    uint64_t* keys = nullptr; uint32_t* hamming = nullptr; uint16_t* prefix_bits = nullptr; uint32_t* count = nullptr;
    uint32_t* freq = nullptr; uint32_t* collisions = nullptr;
    ScoreSink* sink = nullptr;
    static SearchOut lists(uint64_t* k, uint32_t* h, uint16_t* p, uint32_t* c) { SearchOut o; o.keys = k; o.hamming = h; o.prefix_bits = p; o.count = c; return o; }
    static SearchOut doc_freq(uint32_t* freq, uint32_t* collisions = nullptr) { SearchOut o; o.freq = freq; o.collisions = collisions; return o; }
    static SearchOut to_sink(ScoreSink* sink) { SearchOut o; o.sink = sink; return o; }
};
// The speculation steps that search_locked and isccsearch_search_many share (LockedBatch::choose explains the kinds); record_hint is the third.
// choose: a segment's hints serve ordinary top-k searches of a table whose ONE segment it is, and that it can give k rows
// (skip_one_launch: a segment small enough for the one-launch search -- Batch::tiny -- has nothing to gain from a radius: it is exact in that launch either way)
static bool hints_serve(const isccsearch_handle* h, const Segment* seg, uint32_t k, int radius, bool skip_one_launch) {
    if (!seg || radius >= 0 || k > seg->n) return false;
    const bool one_launch = seg->n <= (uint64_t)h->opt.tiny_rows && seg->n < (uint64_t)h->opt.mfma_min_rows && seg->n <= (uint64_t)h->opt.candidate_cap;
    return !(skip_one_launch && one_launch);
}
// choose: the hint a batch speculates under now, or -1.  (Asking counts a backed-off hint's skipped batches down: once per batch, and last.)
static int ready_hint(const isccsearch_handle* h, Segment* seg, uint32_t m, uint32_t len, uint32_t k, bool allowed) {
    return allowed && h->opt.speculate && seg->hint(m, len).ready(k) ? (int)seg->hint(m, len).tau : -1;
}
// verify: the verdict is counted, and a miss backs the hint off
static bool count_verdict(isccsearch_handle* h, HintBackoff& hint, bool ok) {
    if (ok) h->stats.spec_hits += 1;
    else { h->stats.spec_misses += 1; hint.miss(); }
    return ok;
}
// accounting (tools/probe_candidate_path.py, option "count_candidates"): how many candidates the scan appended for a batch
static int appended(isccsearch_handle* h, const Batch& b, uint64_t& sum) {
    std::vector<uint32_t> hc((size_t)b.nq_pad * isk::CNT_STRIDE);
    HIPOK(hipMemcpyAsync(hc.data(), h->d_cnt.p, hc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < b.nq; ++i) sum += hc[(size_t)i * isk::CNT_STRIDE];
    return 0;
}

enum class Spec { none, radius, self_hint, tight, ratio };
// What a search_locked call gives each of its batches
struct LockedCall {
    isccsearch_handle* h; Table& t; uint32_t k; int radius; const SearchOut& out;
    bool may_speculate;                     // false: the rerun of a request whose speculative pass just missed (isccsearch_search_many)
    const std::vector<uint32_t>& order;     // the call's queries, grouped by byte length
    const std::vector<uint64_t>& hq;        // this batch's query words [m][max_words]
};
// One batch of a search_locked call -- the queries order[pos .. pos + m), all of `len` bytes -- and its steps; run() is their order.
// Both mirrors of the result block are sized before it is made.
struct LockedBatch : LockedCall {
    const uint32_t pos, m, len;
    const ResultBlock blk;
    ScoreSink* const sink;
    const uint32_t segments;
    const bool one_copy;                // flags ride in the block: results leave in ONE copy
    // ... or in none: select_kernel writes a small block straight into the pinned mirror (page-locked memory is mapped
    // into the device's address space), so the host only synchronises.  A device->host copy costs ~25 us of queue
    // hand-over after the kernel, more than the 240 bytes per query take to cross PCIe as plain stores.  Large blocks
    // (big k x many queries) keep the DMA copy.
    const bool direct;
    unsigned char* const d_base;        // the block the kernels write: the pinned mirror itself when direct
    const isk::Record* const p_rec; const uint32_t* const p_cnt;    // records and counts of the pinned mirror
    Batch batch;
    Segment* const seg;                 // radius / self_hint / tight: the table's only segment (else nullptr)
    bool hintable = false, mhintable = false;   // this batch's class keeps a hint with its segment / (several segments) with its table
    Spec spec = Spec::none;
    int tau = -1;                       // radius / self_hint / tight: the hint this batch speculates under
    bool spec_ok = false;               // the speculative step stands: its lists are the answer
    bool handed_out = false;            // (tight, repaired) the lists are in the caller's arrays already

    LockedBatch(const LockedCall& c, uint32_t pos_, uint32_t m_, uint32_t len_, const ResultBlock& b)
        : LockedCall(c), pos(pos_), m(m_), len(len_), blk(b), sink(c.out.sink), segments(c.t.segments()), one_copy(segments == 1 && !c.out.freq),
          direct(one_copy && b.bytes() <= DIRECT_RESULT_BYTES && !sink), d_base(direct ? c.h->p_block.p : c.h->d_block.p),
          p_rec(b.records(c.h->p_block.p)), p_cnt(b.counts(c.h->p_block.p)),
          // (a sink keeps the records on the device)
          batch(c.h, c.t, m_, len_, c.k, sink ? sink->records(pos_, c.k) : b.records(d_base), b.counts(d_base)), seg(c.t.sole_segment()) {
        batch.radius = radius;
        if (sink) { batch.d_out_rows = sink->rows(pos, k); batch.d_out_kth = blk.extra(d_base); }
        if (one_copy) { batch.d_flags = blk.flags(d_base); batch.h_flags = blk.flags(h->p_block.p); }
    }

    // (tight: the batch's one job would take the single pass, and that pass is ONE launch of mfma_pack3_kernel)
    bool runs_pack3() { batch.plan(hq.data()); return batch.jobs.size() == 1 && batch.path(batch.jobs[0]) == Batch::Path::single && batch.pack3_pass(batch.jobs[0]); }
    // choose: the kind of speculation and the value it runs under
    void choose() {
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
        //   tight      LARGER batches whose pass would run mfma_pack3_kernel (one-word codes, more than four query groups; host lists).
        //              That kernel's fold flags lanes against ONE threshold per wave, the largest of its chunk + 1, and per-query
        //              thresholds only choose among the flagged rows: they save no fold work, while keeping them live costs 9-10 % of
        //              the pass (profiles/r05_pack3_ab.txt).  So the pass runs as a RANGE-LIMITED search under one radius for every
        //              query: the worst k-th distance the class last ended at (the hint without its margin, + RADIUS_BATCH_SLACK).
        //              Up to RADIUS_BATCH_MAX_REPAIRS queries that find fewer than k rows there are asked again, alone, under the
        //              whole hint and their lists spliced in; more of them send the batch through the self_hint pass.  Either way
        //              the step stands exactly when every query has k rows within the hint and no list overflowed, as with self_hint.
        // radius / self_hint / tight: an ordinary top-k search over ONE segment that has been searched with this k before
        hintable = hints_serve(h, seg, k, radius, /*skip_one_launch=*/true) && !out.freq && one_copy;
        const bool small_batch = hintable && m <= (uint32_t)h->opt.spec_max_queries;
        tau = ready_hint(h, seg, m, len, k, hintable && may_speculate && (small_batch || h->opt.self_hint));
        if (tau >= 0) {
            if (small_batch) { spec = Spec::radius; batch.radius = tau; }
            else if (h->opt.radius_batches && !sink && runs_pack3()) {
                spec = Spec::tight;
                batch.radius = std::max(0, tau - (int)Segment::SpecHint::margin(k) + RADIUS_BATCH_SLACK);
            } else { spec = Spec::self_hint; batch.self_hint = tau; }
        }
        mhintable = segments > 1 && radius < 0 && !out.freq && (m <= (uint32_t)h->opt.spec_max_queries || h->opt.self_hint) && k <= t.total;
        if (mhintable && h->opt.speculate && may_speculate && t.mhint(m, len).ready(k)) {
            spec = Spec::ratio;
            batch.radius_ratio = t.mhint(m, len).ratio + 1.0 / 32.0;      // the margin: 2 bits of 64, 8 of 256
            batch.ratio_starts_self = m > (uint32_t)h->opt.spec_max_queries;             // larger batches: each segment's single pass STARTS under it
        }
    }
    // queue results: whatever of the block is not yet where the host reads it, behind the kernels that turn lists into what the caller asked for
    int queue_results() {
        if (out.freq) {
            // only the distinct-asset count of every list leaves the device
            int rf;
            if ((rf = h->d_freq.ensure(m))) return rf;
            isk::DistinctParams dp{batch.d_out, batch.d_out_cnt, h->d_freq.p, k, (uint32_t)t.key_words};
            hipLaunchKernelGGL(isk::distinct_kernel, dim3(m), dim3(isk::BLOCK), 0, h->stream, dp);
            HIPOK(hipGetLastError());
            if (out.collisions) HIPOK(hipMemcpyAsync(blk.extra(h->p_block.p), batch.d_out_cnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            HIPOK(hipMemcpyAsync(blk.counts(h->p_block.p), h->d_freq.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            return 0;
        }
        if (direct) return 0;                                  // already written where the host reads it
        if (sink) {
            // the host gets counts, flags, k-th distances and info
            HIPOK(sink->queue_behind_select(pos, m, k, batch.d_out_cnt, blk.info(d_base), h->stream));
            HIPOK(hipMemcpyAsync(h->p_block.p, h->d_block.p, blk.bytes(), hipMemcpyDeviceToHost, h->stream));
            return 0;
        }
        HIPOK(hipMemcpyAsync(h->p_block.p, h->d_block.p, blk.bytes_with(one_copy ? batch.flag_words() : 0), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }
    // settle: merge, flags, results, one synchronisation
    int settle() {
        int rs;
        if ((rs = batch.merge())) return rs;
        if ((rs = batch.copy_flags())) return rs;
        if ((rs = queue_results())) return rs;
        HIPOK(hipStreamSynchronize(h->stream));
        return 0;
    }
    double worst_ratio() const {                 // worst k-th NPHD of the merged lists; < 0: some query holds fewer than k rows
        double worst = 0.0;
        for (uint32_t i = 0; i < m; ++i) {
            if (p_cnt[i] < k) return -1.0;
            const isk::Record& r = p_rec[(size_t)i * k + k - 1];
            worst = std::max(worst, r.prefix_bits ? (double)r.hamming / (double)r.prefix_bits : 0.0);
        }
        return worst;
    }
    // ratio: every query holds k rows and its k-th lies inside the radius of its own compared prefix -- in bits, as the segments listed
    // their rows.  (Not worst_ratio() <= radius_ratio: h / 192 and ratio + 1/32 round apart as doubles, and a k-th row at exactly
    // 11/192 + 1/32 = 17/192, which its segment lists, was taken for a miss.)
    bool kth_within_ratio() const {
        for (uint32_t i = 0; i < m; ++i) {
            if (p_cnt[i] < k) return false;
            const isk::Record& r = p_rec[(size_t)i * k + k - 1];
            if ((int)r.hamming > batch.ratio_bits((int)r.prefix_bits)) return false;
        }
        return true;
    }
    // repair (tight): the queries in `short_q` (positions in this batch) alone, as a range-limited search under the whole hint -- which
    // neither reads nor updates a hint.  spec_ok: each of them holds k rows now and no list overflowed; their lists are spliced in.
    int repair(const std::vector<uint32_t>& short_q) {
        int rr;
        // The main pass's lists leave first: the repair reuses p_block, d_block and d_cnt (as pass 3a of isccsearch_search_many
        // hands every deferred result out before pass 3b runs)
        unpack_records(p_rec, p_cnt, m, k, t.key_words, &order[pos], out.keys, out.hamming, out.prefix_bits, out.count);
        uint64_t cand = 0;
        if (h->opt.count_candidates && (rr = appended(h, batch, cand))) return rr;
        const uint32_t ns = (uint32_t)short_q.size();
        std::vector<uint64_t> rq((size_t)ns * t.max_words);
        std::vector<uint32_t> dest(ns);
        for (uint32_t j = 0; j < ns; ++j) {
            memcpy(&rq[(size_t)j * t.max_words], &hq[(size_t)short_q[j] * t.max_words], (size_t)t.max_words * 8);
            dest[j] = order[pos + short_q[j]];
        }
        // its block {records [ns][k] | counts [ns] | flags} is smaller than the batch's: it fits both mirrors as they are
        const ResultBlock rblk{ns, k};
        const bool r_direct = rblk.bytes() <= DIRECT_RESULT_BYTES;
        unsigned char* const r_base = r_direct ? h->p_block.p : h->d_block.p;
        const uint32_t* const rp_cnt = rblk.counts(h->p_block.p);
        Batch rb(h, t, ns, len, k, rblk.records(r_base), rblk.counts(r_base));
        rb.radius = tau;
        rb.on_matrix_cores = true;
        rb.d_flags = rblk.flags(r_base);
        rb.h_flags = rblk.flags(h->p_block.p);
        if ((rr = rb.begin(rq.data()))) return rr;
        if (!r_direct) HIPOK(hipMemcpyAsync(h->p_block.p, h->d_block.p, rblk.bytes_with(rb.flag_words()), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        if (h->opt.count_candidates && (rr = appended(h, rb, cand))) return rr;
        spec_ok = rb.complete(rp_cnt, seg->n);
        if (!spec_ok) return 0;         // (the ordinary pass answers the whole batch again, and is what gets counted)
        unpack_records(p_rec, rp_cnt, ns, k, t.key_words, dest.data(), out.keys, out.hamming, out.prefix_bits, out.count);
        handed_out = true;
        h->stats.candidates += cand;
        h->stats.spec_repairs += ns;
        return 0;
    }
    // verify: does the settled speculative step stand (spec_ok)?
    int verify() {
        int rc;
        // (ratio: a row outside a radius lies at floor(ratio x bits) + 1 bits or beyond, strictly farther than any k-th row inside its own)
        if (spec == Spec::ratio) spec_ok = batch.complete(p_cnt, k) && kth_within_ratio();
        else if (spec != Spec::tight) spec_ok = batch.complete(p_cnt, seg->n);
        else {
            std::vector<uint32_t> short_q;          // (hintable: k <= rows, so a query is short of k)
            for (uint32_t i = 0; i < m; ++i) if (p_cnt[i] < k) short_q.push_back(i);
            if (batch.any_flag()) spec_ok = false;
            else if (short_q.empty()) spec_ok = true;
            else if (short_q.size() <= RADIUS_BATCH_MAX_REPAIRS) { if ((rc = repair(short_q))) return rc; }
            else {
                // too many for one small pass: the hinted single pass for the whole batch, whose own check gives the verdict
                batch.radius = radius; batch.self_hint = tau;
                if ((rc = batch.begin(hq.data()))) return rc;
                if ((rc = settle())) return rc;
                spec_ok = batch.used_hint && batch.complete(p_cnt, seg->n);
            }
        }
        return 0;
    }
    // record: candidate accounting, and where this batch's lists ended -- the next batch of its class starts there (+ the hint's margin)
    int record() {
        int rc;
        if (h->opt.count_candidates && batch.jobs.size() == 1) {
            // (a repaired step has counted both of its passes before the second reused the counters)
            if (!handed_out && (rc = appended(h, batch, h->stats.candidates))) return rc;
            h->stats.candidate_batches += 1;
        }
        if (handed_out) {
            // (the pinned block holds the repair's lists by now: the batch's worst k-th distance, repaired queries included, is in the caller's arrays)
            uint32_t worst = 0;
            for (uint32_t i = 0; i < m; ++i) {
                const size_t dq = order[pos + i];
                if (out.count[dq]) worst = std::max(worst, out.hamming[dq * k + out.count[dq] - 1]);
            }
            record_hint(seg->hint(m, len), spec_ok, k, worst);
        } else if (hintable && !batch.jobs.empty()) record_hint(seg->hint(m, len), spec_ok, m, k, p_cnt, p_rec, sink ? blk.extra(h->p_block.p) : nullptr);
        if (mhintable) {
            const double worst = worst_ratio();
            if (spec_ok) t.mhint(m, len).hit(worst);
            else if (worst >= 0.0) t.mhint(m, len).seed(k, worst);
        }
        return 0;
    }
    // hand out: the sink's bookkeeping, document frequencies (and collisions), or the lists
    void hand_out() {
        const bool none = batch.jobs.empty();
        if (sink) {
            if (!none) sink->take(pos, m, k, p_cnt, blk.info(h->p_block.p));
        } else if (out.freq) {
            for (uint32_t i = 0; i < m; ++i) out.freq[order[pos + i]] = none ? 0 : p_cnt[i];
            if (out.collisions) for (uint32_t i = 0; i < m; ++i) out.collisions[order[pos + i]] = none ? 0 : blk.extra(h->p_block.p)[i];
        } else if (!handed_out) {
            unpack_records(p_rec, p_cnt, m, k, t.key_words, &order[pos], out.keys, out.hamming, out.prefix_bits, out.count);
        }
    }
    int run() {
        int rc;
        choose();
        if ((rc = batch.begin(hq.data()))) return rc;
        if (spec == Spec::ratio && !batch.multi) {          // (every non-empty segment is a job: cannot happen; never answer unverified)
            spec = Spec::none;
            batch.radius_ratio = -1.0;
            if ((rc = batch.begin(hq.data()))) return rc;
        }
        if (spec == Spec::self_hint && !batch.used_hint) spec = Spec::none;     // (no job took the single pass: nothing to verify)
        if (spec != Spec::none) {
            if ((rc = settle()) || (rc = verify())) return rc;
            HintBackoff& hint = spec == Spec::ratio ? static_cast<HintBackoff&>(t.mhint(m, len)) : seg->hint(m, len);
            if (!count_verdict(h, hint, spec_ok)) {
                // on a miss: the ordinary pass
                batch.radius = radius; batch.self_hint = -1; batch.used_hint = false; batch.radius_ratio = -1.0;
                if ((rc = batch.begin(hq.data()))) return rc;
            }
        }
        if (!spec_ok && (rc = batch.finish(hq.data(), [this] { return queue_results(); }))) return rc;
        if ((rc = record())) return rc;
        hand_out();
        return 0;
    }
};

// The search itself; h->mu is held by the caller.  radius >= 0: range-limited search (fixed threshold).
static int search_locked(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words, const uint8_t* q_nbytes, uint32_t k,
                         int radius, const SearchOut& out, bool may_speculate = true) {
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
    const LockedCall call{h, t, k, radius, out, may_speculate, order, hq};
    uint32_t pos = 0;
    while (pos < nq) {
        const uint32_t len = qlen(order[pos]);
        uint32_t end = pos;
        while (end < nq && end - pos < QB_MAX && qlen(order[end]) == len) ++end;
        const uint32_t m = end - pos;
        hq.resize((size_t)m * t.max_words);
        for (uint32_t i = 0; i < m; ++i)
            memcpy(&hq[(size_t)i * t.max_words], q_words + (size_t)order[pos + i] * t.max_words, (size_t)t.max_words * 8);
        // (+ the lists' lengths when a document-frequency call also wants them; a sink keeps the records on the device and gets the
        //  k-th distances and the scoring kernels' info words)
        const ResultBlock blk{m, k, !out.sink, out.collisions || out.sink, out.sink != nullptr};
        if ((rc = h->d_block.ensure(blk.bytes()))) return rc;
        if ((rc = h->p_block.ensure(blk.bytes()))) return rc;
        LockedBatch lb(call, pos, m, len, blk);
        if ((rc = lb.run())) return rc;
        pos = end;
    }
    return 0;
}

// Searches arriving from many threads are COMBINED: the reference calls `search` once per query unit from
// FastAPI's thread pool (usearch/index.py:786-806, docs/explanation/architecture.md:120-126), and a
// streaming pass costs the same for one query as for T_q.  The first caller becomes the leader of a round and
// takes EVERY request waiting on the handle; run_combined groups them by (table, k) and runs each group as ONE
// batch; the others sleep until their slice of the results has been written.  A request that arrives while a
// round runs waits for the next one.  A single-threaded caller pays nothing for this.
struct PendingSearch {
    uint32_t table, nq, k;
    const uint64_t* q_words;
    const uint8_t* q_nbytes;
    SearchOut out;      // (its lists)
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
            r->rc = search_locked(h, r->table, r->nq, r->q_words, r->q_nbytes, r->k, -1, r->out);
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
        const int rg = search_locked(h, reqs[i]->table, (uint32_t)total, qw.data(), qn.empty() ? nullptr : qn.data(), k, -1,
                                     SearchOut::lists(okeys.data(), oh.data(), op.data(), oc.data()));
        const std::string eg = rg ? g_last_error : std::string();
        off = 0;
        for (size_t j : ok) {
            PendingSearch* r = reqs[j];
            r->rc = rg;
            r->err = eg;
            if (!rg) {
                memcpy(r->out.keys, &okeys[off * k * KW], (size_t)r->nq * k * KW * 8);
                memcpy(r->out.hamming, &oh[off * k], (size_t)r->nq * k * 4);
                memcpy(r->out.prefix_bits, &op[off * k], (size_t)r->nq * k * 2);
                memcpy(r->out.count, &oc[off], (size_t)r->nq * 4);
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
    if (int rc = check_count(k)) return rc;
    if (nq == 0) return 0;
    if (!q_words || !out_keys || !out_hamming || !out_prefix_bits || !out_count) return fail(-EINVAL, "NULL argument");
    PendingSearch me;
    me.table = table; me.nq = nq; me.k = k; me.q_words = q_words; me.q_nbytes = q_nbytes;
    me.out = SearchOut::lists(out_keys, out_hamming, out_prefix_bits, out_count);
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

struct ManySlot {            // a deferred request of isccsearch_search_many
    std::unique_ptr<Batch> batch;
    std::vector<uint64_t> hq;
    size_t off = 0;         // its result block in p_block ...
    ResultBlock blk{};      // ... and that block's layout (in d_block every request's block starts at 0)
    Segment* seg = nullptr;
    bool small = false;     // its class keeps a hint with the segment
    int tau = -1;           // >= 0: the hint it speculates under
    uint32_t len = 0;       // compared prefix length of the request (the hint is kept per length)
};
// a request of isccsearch_search_many with queries, checked; on success `tp` is its table
static int check_request(isccsearch_handle* h, const isccsearch_request& r, Table*& tp) {
    if (int rk = check_count(r.k)) return rk;
    if (r.max_hamming > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", r.max_hamming);
    if (!r.q_words || !r.out_keys || !r.out_hamming || !r.out_prefix_bits || !r.out_count) return fail(-EINVAL, "NULL argument");
    const int rc = get_table(h, r.table, tp);
    return rc ? rc : check_query_lengths(*tp, r.nq, r.q_nbytes);
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
    std::vector<ManySlot> slots(n);
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
        Table* tp;
        if (int rc = check_request(h, r, tp)) { reject(r, rc); continue; }
        if (tp->segments() != 1 || first_other_length(*tp, r.nq, r.q_nbytes) != r.nq || r.nq > QB_MAX) continue;     // ordinary path below
        deferred[i] = true;
        slots[i].blk = ResultBlock{r.nq, r.k};
        slots[i].off = block_total;
        block_total += slots[i].blk.slice_bytes();
        block_max = std::max(block_max, slots[i].blk.slice_bytes());
        pq_words += staged_words_for(r.nq);
    }
    int rc;
    if ((rc = wait_staged(h))) return rc;
    if ((rc = h->p_queries.ensure(pq_words))) return rc;
    if ((rc = h->p_block.ensure(block_total))) return rc;
    if ((rc = h->d_block.ensure(block_max))) return rc;

    // pass 2: enqueue
    size_t pq_off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!deferred[i]) continue;
        isccsearch_request& r = reqs[i];
        Table& t = *h->tables[r.table];
        ManySlot& sl = slots[i];
        sl.len = t.metric == ISCCSEARCH_METRIC_NPHD ? r.q_nbytes[0] : (uint32_t)t.max_bytes;
        sl.batch.reset(new Batch(h, t, r.nq, sl.len, r.k, sl.blk.records(h->d_block.p), sl.blk.counts(h->d_block.p)));
        Batch& b = *sl.batch;
        b.radius = r.max_hamming < 0 ? -1 : r.max_hamming;
        // small top-k batches: the speculative single pass of search_locked (LockedBatch::choose), verified in pass 3a.  Not as there:
        // the hints of a segment small enough for the one-launch search are kept and used too, ...
        sl.seg = t.sole_segment();
        sl.small = hints_serve(h, sl.seg, r.k, b.radius, /*skip_one_launch=*/false) && r.nq <= (uint32_t)h->opt.spec_max_queries;
        // ... and a request speculates by radius or not at all: one above spec_max_queries neither starts its pass under a hint nor seeds one
        sl.tau = ready_hint(h, sl.seg, r.nq, sl.len, r.k, /*allowed=*/sl.small);
        if (sl.tau >= 0) b.radius = sl.tau;
        b.pq_off = pq_off;
        b.d_flags = sl.blk.flags(h->d_block.p);
        b.h_flags = sl.blk.flags(h->p_block.p + sl.off);
        pq_off += staged_words_for(r.nq);
        sl.hq.assign(r.q_words, r.q_words + (size_t)r.nq * t.max_words);
        h->stats.searches += 1;
        h->stats.queries += r.nq;
        if ((rc = b.begin(sl.hq.data()))) return rc;
        HIPOK(hipMemcpyAsync(h->p_block.p + sl.off, h->d_block.p, sl.blk.bytes_with(b.flag_words()), hipMemcpyDeviceToHost, h->stream));
    }
    HIPOK(hipStreamSynchronize(h->stream));

    // pass 3a: hand out EVERY deferred result first.  The ordinary pipeline below stages its own results in p_block
    // from offset 0 (and may reallocate it), so no deferred slice may still be unread when it runs.
    std::vector<bool> ordinary(n, false), respec(n, true);      // respec: the ordinary rerun may itself speculate (not after a miss)
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_request& r = reqs[i];
        if (r.status || r.nq == 0) continue;
        if (!deferred[i]) { ordinary[i] = true; continue; }
        ManySlot& sl = slots[i];
        Batch& b = *sl.batch;
        const isk::Record* p_rec = sl.blk.records(h->p_block.p + sl.off);
        const uint32_t* p_cnt = sl.blk.counts(h->p_block.p + sl.off);
        // (after a miss the ordinary path re-seeds the radius)
        if (sl.tau >= 0 && !count_verdict(h, sl.seg->hint(r.nq, sl.len), b.complete(p_cnt, sl.seg->n))) { ordinary[i] = true; respec[i] = false; continue; }
        if (b.any_flag()) { ordinary[i] = true; continue; }   // rare: exact fallback through the normal path
        if (sl.small && !b.jobs.empty()) record_hint(sl.seg->hint(r.nq, sl.len), sl.tau >= 0, r.nq, r.k, p_cnt, p_rec, nullptr);
        unpack_records(p_rec, p_cnt, r.nq, r.k, h->tables[r.table]->key_words, nullptr, r.out_keys, r.out_hamming, r.out_prefix_bits, r.out_count);
    }
    // pass 3b: overflowed and non-deferred requests run the ordinary pipeline
    for (uint32_t i = 0; i < n; ++i) {
        if (!ordinary[i]) continue;
        isccsearch_request& r = reqs[i];
        if (!deferred[i]) h->stats.searches += 1;
        rc = search_locked(h, r.table, r.nq, r.q_words, r.q_nbytes, r.k, r.max_hamming < 0 ? -1 : r.max_hamming,
                           SearchOut::lists(r.out_keys, r.out_hamming, r.out_prefix_bits, r.out_count), /*may_speculate=*/respec[i]);
        if (rc) reject(r, rc);
    }
    return first_error;
}

int isccsearch_search_within(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                             const uint8_t* q_nbytes, uint32_t k, uint32_t max_hamming,
                             uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (int rc = check_count(k)) return rc;
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %u exceeds 256", max_hamming);
    if (nq == 0) return 0;
    if (!q_words || !out_keys || !out_hamming || !out_prefix_bits || !out_count) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->stats.searches += 1;
    return search_locked(h, table, nq, q_words, q_nbytes, k, (int)max_hamming, SearchOut::lists(out_keys, out_hamming, out_prefix_bits, out_count));
}

int isccsearch_doc_freq(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                        const uint8_t* q_nbytes, uint32_t dup_limit, uint32_t* out_freq) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1 || dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u outside 1..ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (nq == 0) return 0;
    if (!q_words || !out_freq) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->stats.searches += 1;
    return search_locked(h, table, nq, q_words, q_nbytes, dup_limit, 0, SearchOut::doc_freq(out_freq));
}

int isccsearch_doc_freq_counted(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                const uint8_t* q_nbytes, uint32_t dup_limit, uint32_t* out_freq, uint32_t* out_collisions) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1 || dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u outside 1..ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (nq == 0) return 0;
    if (!q_words || !out_freq || !out_collisions) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->stats.searches += 1;
    return search_locked(h, table, nq, q_words, q_nbytes, dup_limit, 0, SearchOut::doc_freq(out_freq, out_collisions));
}
}  // extern "C"
