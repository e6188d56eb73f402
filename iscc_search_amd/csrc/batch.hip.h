// batch.hip.h -- the launcher every search entry point goes through (same translation unit as isccsearch.hip): the kernel dispatch, the scan
// grid, the profile brackets and Batch, the search pipeline of one batch of equal-length queries -- one function per search path.
// Needs the common types, the options and the handle of isccsearch.hip.

// ------------------------------------------------------------------------------------------
// kernel dispatch
// ------------------------------------------------------------------------------------------
// only the non-temporal variant of scan_kernel (its last template argument) is instantiated: plain loads measured no faster
//  and every extra variant costs build time
void launch_scan(int W, bool mask, int tq, int mode, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    // (the XOR + popcount kernels have no MODE_SELF, which Batch::scan refuses: that mode launches nothing here)
    auto with_tq = [&](auto&& f) { if (tq == 8) f(isk::int_c<8>{}); else f(isk::int_c<16>{}); };
    if (W == 1 && !mask) {   // whole 64-bit codes: the kernel picks its fast path per query group (ScanParams::fold_tau)
        isk::with_mode(mode, [&](auto m) { with_tq([&](auto t) {
            if constexpr (decltype(m)::value != isk::MODE_SELF) hipLaunchKernelGGL((isk::scan_adapt_kernel<decltype(t)::value, decltype(m)::value>), grid, dim3(isk::BLOCK), 0, st, p);
        }); });
        return;
    }
    isk::with_words(W, [&](auto w) {
        auto masked = [&](auto mk) { with_tq([&](auto t) { isk::with_mode(mode, [&](auto m) {
            constexpr int WORDS = decltype(w)::value, MODE = decltype(m)::value;
            constexpr bool MASK = decltype(mk)::value;
            // (W = 1 here is shorter than 64 bits: whole words went above)
            if constexpr (MODE != isk::MODE_SELF && (WORDS > 1 || MASK)) hipLaunchKernelGGL((isk::scan_kernel<WORDS, MASK, decltype(t)::value, MODE>), grid, dim3(isk::BLOCK), 0, st, p);
        }); }); };
        if (mask) masked(std::true_type{}); else masked(std::false_type{});
    });
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
    int ratio_bits(int bits) const { return std::min(bits, (int)std::floor(radius_ratio * bits + 1e-9)); }
    int ratio_bits(const Job& j) const { return ratio_bits(8 * (int)j.pbytes); }
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
    // One job on its way through its path: its parameter blocks, the fixed threshold of a range-limited pass (or -1), and whether the
    // histogram behind sp.ghist is zeroed and in use
    struct Run { const Job& j; Ctx c; int radius; bool hist_live = false; };

    // select_kernel and tiny_search_kernel are instantiated per (key words, "the segment rows of the records too"): f(key words, rows)
    template <typename F>
    void with_record_form(const isk::SelectParams& sl, F&& f) const {
        auto keyed = [&](auto rows) { isk::with_key_words(t.key_words, [&](auto kw) { f(kw, rows); }); };
        if (sl.out_rows) keyed(std::true_type{}); else keyed(std::false_type{});
    }
    template <int NT>
    void launch_select_nt(const isk::SelectParams& sl, uint32_t blocks) const {
        with_record_form(sl, [&](auto kw, auto rows) { hipLaunchKernelGGL((isk::select_kernel<decltype(kw)::value, decltype(rows)::value, NT>), dim3(blocks), dim3(NT), sel_lds, h->stream, sl); });
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
        with_record_form(sl, [&](auto kw, auto rows) { hipLaunchKernelGGL((isk::tiny_search_kernel<decltype(kw)::value, decltype(rows)::value, NT>), dim3(nq), dim3(NT), sel_lds, h->stream, tp, sl, iq); });
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
    // The path a job takes through begin() -- the only place that combines tiny(), job_radius() and single_pass():
    //   tiny     ONE launch answers a segment of few rows
    //   radius   range-limited search: the threshold is given, so one streaming pass collects everything
    //   single   Large batches take ONE pass on the matrix cores with self-tightening thresholds (MODE_SELF).
    //   levels   (The XOR + popcount kernels keep the levels: their resident blocks cover ~4 M rows -- 16 M by the time a second
    //            tile could see a new threshold -- before any update reaches them, and fresh thresholds must be read past the
    //            per-XCD L2s (sc1 / glc), where 8 192 waves hammering one line serialise: measured 0.24-0.53 ms for 1-8
    //            queries over 100 M rows against 0.10 ms for the collect pass of the level design.)
    enum class Path { tiny, radius, single, levels };
    Path path(const Job& j) const {
        if (tiny(j)) return Path::tiny;
        if (job_radius(j) >= 0) return Path::radius;
        return single_pass(j) ? Path::single : Path::levels;
    }
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
    // the sizes of the batch and every scratch buffer it writes
    int reserve() {
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
        return 0;
    }
    // the batch's slice of the pinned staging, once stage() has filled it: [nq_pad][4]
    const uint64_t* staged() const { return h->p_queries.p + pq_off; }
    bool all_tiny() const {
        for (const Job& j : jobs) if (!tiny(j)) return false;
        return true;
    }
    // (a range-limited search of <= 16 queries over one segment -- the speculative single pass of search_locked -- carries its
    //  queries in the ARGUMENTS of its first kernel, which writes them to d_queries: one stream operation less, ~8 us of 170)
    bool inline_queries() const { return !all_tiny() && radius >= 0 && nq_pad <= isk::INLINE_QUERIES && jobs.size() == 1; }
    // (... and so do the one-launch searches of tiny segments: when every job of the batch is one, nothing is uploaded at all)
    bool tiny_inline() const { return all_tiny() && nq_pad <= isk::INLINE_QUERIES; }
    int stage(const uint64_t* hq) {
        // stage queries through pinned memory: [nq_pad][4], padded words zero
        int rc;
        if ((rc = wait_staged(h))) return rc;
        if ((rc = h->p_queries.ensure(pq_off + (size_t)nq_pad * 4))) return rc;   // (no-op when the caller pre-sized it)
        uint64_t* const pq = h->p_queries.p + pq_off;
        memset(pq, 0, (size_t)nq_pad * 4 * 8);
        for (uint32_t q = 0; q < nq; ++q)
            for (int w = 0; w < t.max_words; ++w) pq[(size_t)q * 4 + w] = hq[(size_t)q * t.max_words + w];
        if (!inline_queries() && !tiny_inline()) HIPOK(hipMemcpyAsync(h->d_queries.p, pq, (size_t)nq_pad * 4 * 8, hipMemcpyHostToDevice, h->stream));
        if (mark_overflow) { HIPOK(hipEventRecord(h->ev_staged, h->stream)); h->ev_staged_pending = true; }
        return 0;
    }
    int begin(const uint64_t* hq) {
        plan(hq);
        used_self = false;
        if (jobs.empty()) {
            HIPOK(hipMemsetAsync(d_out_cnt, 0, nq * sizeof(uint32_t), h->stream));
            return 0;
        }
        int rc;
        if ((rc = reserve())) return rc;
        if ((rc = stage(hq))) return rc;
        for (size_t ji = 0; ji < jobs.size(); ++ji) {
            Run run{jobs[ji], make_ctx(ji), job_radius(jobs[ji])};
            switch (path(run.j)) {
                case Path::tiny: rc = run_tiny(run); break;
                case Path::radius: rc = run_radius(run); break;
                case Path::single: used_self = true; rc = run_single(run); break;
                case Path::levels: rc = run_levels(run); break;
            }
            if (rc) return rc;
        }
        return 0;
    }

    // the statistics of one collect launch over `rows` rows, which cross the memory system `passes` times
    void count_scan(const Job& j, uint64_t rows, uint32_t passes) {
        h->stats.scan_launches += 1;
        h->stats.scan_passes += passes;
        h->stats.scan_bytes += rows * 8 * j.W * passes;
        h->stats.scan_pair_words += rows * (uint64_t)nq * j.W;
    }
    int run_tiny(Run& run) {
        const Job& j = run.j;
        const Segment& s = *j.seg;
        // ONE launch: distances of every row, candidate list, select -- exact, nothing to verify or to repeat
        isk::TinyParams tp{};
        set_cols(tp.col, s, j.W);
        tp.queries = h->d_queries.p; tp.cand = h->d_cand.p; tp.mask_last = j.mask_last; tp.n_rows = (uint32_t)s.n; tp.W = j.W;
        tp.radius = run.radius; tp.use_inline = tiny_inline() ? 1u : 0u;
        isk::InlineQueries iq;
        if (tp.use_inline) memcpy(iq.w, staged(), (size_t)nq_pad * 4 * 8);
        else memset(iq.w, 0, sizeof iq.w);
        hipEvent_t e1 = nullptr;
        int rc;
        if ((rc = profile_begin(h, e1))) return rc;
        // (a block walks ALL rows: 1 024 threads whenever the batch leaves the chip room for them, and for the sort buffers select_kernel gives them)
        const bool wide = (s.n > 2048 && nq <= (uint32_t)h->cus / 2) || run.c.sl.P >= 2 * (uint64_t)h->opt.select_wide_from || (run.c.sl.P >= (uint64_t)h->opt.select_wide_from && nq <= (uint32_t)h->cus / 2);
        if (wide) launch_tiny_nt<1024>(tp, run.c.sl, iq);
        else launch_tiny_nt<isk::BLOCK>(tp, run.c.sl, iq);
        HIPOK(hipGetLastError());
        if ((rc = profile_end(h, e1))) return rc;
        count_scan(j, s.n, nq);
        return 0;
    }

    // the collect pass over rows [from, n) within the thresholds in force.  With more than one query group the
    // rows are taken in STRETCHES that fit the Infinity Cache (option "stretch_mb", default 128 of its
    // 256 MB): all groups of a launch walk the same stretch, so it comes out of HBM once and out of the
    // caches for every further group -- the pass is then bound by the VALU, not by HBM.
    int collect(Run& run, uint64_t from, bool self = false) {
        const Job& j = run.j;
        const Segment& s = *j.seg;
        isk::ScanParams& sp = run.c.sp;
        const uint64_t tile_rows = (uint64_t)tile_rows_for((int)j.W);
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
            const bool hist_too = run.radius < 0;
            const bool repick = hist_too && b < s.n && !self;
            if (self) {
                if ((rcl = scan(j, sp, isk::MODE_SELF, false))) return rcl;
            } else if (hist_too) {
                if (!run.hist_live) { HIPOK(hipMemsetAsync(h->d_ghist.p, 0, (size_t)nq_pad * isk::HB * sizeof(uint32_t), h->stream)); run.hist_live = true; }
                if ((rcl = scan(j, sp, isk::MODE_STRETCH, false))) return rcl;
            } else {
                if ((rcl = scan(j, sp, isk::MODE_COLLECT, false))) return rcl;
            }
            if ((rcl = profile_end(h, e1))) return rcl;
            if (repick) {
                isk::PickParams pp{h->d_ghist.p, h->d_bias.p, nq, (uint32_t)std::min<uint64_t>(k, b), h->d_cnt.p, h->d_cand.p, cap};
                hipLaunchKernelGGL(isk::pick_kernel, dim3(nq), dim3(isk::BLOCK), 0, h->stream, pp);
            }
            count_scan(j, rows, groups);
            if (use_mfma(j, rows) || self) h->stats.scan_mfma_launches += 1;
            a = b;
        }
        return 0;
    }

    int run_radius(Run& run) {
        // range-limited search: the threshold is given, so one streaming pass collects everything
        if (inline_queries()) {
            isk::InlineQueries iq;
            memcpy(iq.w, staged(), (size_t)nq_pad * 4 * 8);
            hipLaunchKernelGGL(isk::radius_init_inline_kernel, dim3(1), dim3(isk::BLOCK), 0, h->stream,
                               h->d_bias.p, h->d_cnt.p, nq, nq_pad, 0x7FFFFFFFu - (uint32_t)run.radius, h->d_queries.p, iq);
        } else
        hipLaunchKernelGGL(isk::radius_init_kernel, dim3((nq_pad + isk::BLOCK - 1) / isk::BLOCK), dim3(isk::BLOCK), 0, h->stream,
                           h->d_bias.p, h->d_cnt.p, nq, nq_pad, 0x7FFFFFFFu - (uint32_t)run.radius);
        int rc;
        if ((rc = collect(run, 0))) return rc;
        launch_select(run.c.sl, nq);
        HIPOK(hipGetLastError());
        return 0;
    }

    // rows of a job's bootstrap sample
    // (the single pass appends everything within the bootstrap threshold until the first update arrives -- 3 072 waves x
    //  128 rows at once -- so its sample grows with k (1 024 k rows): 512 k measured 4.39 -> 3.80 ms at k = 256 and 11.9 (list
    //  overflow, retry) -> 5.07 ms at k = 512 against the fixed 65 536, profiles/r03_ab_large_k.txt)
    //  (... and never fewer than k rows: the worst of a shorter sample bounds nothing, and rows beyond it would never be listed)
    uint64_t sample_rows(const Job& j, bool self) const {
        const uint64_t n = j.seg->n;
        return std::min<uint64_t>(n, self ? std::max<uint64_t>(std::max<uint64_t>((uint64_t)h->opt.self_boot_rows, k), std::min<uint64_t>((uint64_t)h->opt.self_boot_per_k * k, n / 8))
                                          : std::max<uint64_t>(BOOT_ROWS, std::min<uint64_t>(65536, 64ull * k)));
    }
    // 1. bootstrap threshold from the first s0 rows
    void boot(Run& run, bool self) {
        const Job& j = run.j;
        isk::BootParams bp{};
        set_cols(bp.col, *j.seg, j.W);
        bp.queries = h->d_queries.p; bp.bias = h->d_bias.p; bp.cnt = h->d_cnt.p; bp.s0 = sample_rows(j, self); bp.nq = nq; bp.k = k; bp.W = j.W; bp.mask_last = j.mask_last;
        bp.thr = self ? h->d_thr.p : nullptr;
        bp.thr_packed = j.pack ? 1u : 0u;          // mfma_pack_kernel keeps (and lowers) its live thresholds packed
        bp.counts = h->d_ghist.p;          // zeroed by the kernel: the running histogram of the levels / the counters of MODE_SELF
        bp.hint = isk::BOOT_NO_HINT;
        run.hist_live = true;
        const int job_hint = self_hint >= 0 ? self_hint : (radius_ratio >= 0 && ratio_starts_self ? ratio_bits(j) : -1);
        if (self && job_hint >= 0) {
            // the threshold a previous batch of this size ended at (+ margin) instead of a sample: no 65 536-row bootstrap, and
            // the pass starts ~6 bits tighter -- without the flood of its first steps.  Verified by the caller.
            bp.hint = (uint32_t)job_hint;
            used_hint = true;
            hipLaunchKernelGGL(isk::boot_kernel, dim3(nq_pad), dim3(64), 0, h->stream, bp);
        } else if (nq_pad > 64) {
            // large batches: four queries per 1 024-thread block share every row load of the sample
            isk::with_words((int)j.W, [&](auto w) { hipLaunchKernelGGL(isk::boot_multi_kernel<decltype(w)::value>, dim3(nq_pad / isk::BOOT_QB), dim3(1024), 0, h->stream, bp); });
        } else {
            // one block per query, and wide ones: a 65 536-row sample is otherwise one block's latency-bound walk
            hipLaunchKernelGGL(isk::boot_kernel, dim3(nq_pad), dim3(1024), 0, h->stream, bp);
        }
    }

    int run_single(Run& run) {
        boot(run, true);
        // 2'. ONE pass over all rows (in cache-sized stretches when several chunks of queries share them):
        //     every wave appends what lies within the live threshold of its query and counts it per distance; the lane
        //     that proves "k rows within t" lowers the threshold for everybody (mfma_scan.hip, MODE_SELF).
        //     No levels, no picks; the lists stay unpruned (~k ln(n / s0) entries + ties + the first steps' flood) and
        //     select_kernel takes the exact top-k.  (boot_kernel has zeroed the counters.)
        int rc;
        if ((rc = collect(run, 0, true))) return rc;
        launch_select(run.c.sl, nq);
        HIPOK(hipGetLastError());
        return 0;
    }

    // how many times the rows seen so far a threshold level streams
    uint64_t level_growth(const Job& j) const {
        uint64_t growth = (groups <= 2 && k <= 64) ? 64 : LEVEL_GROWTH;
        if (use_mfma(j, j.seg->n) && k <= 64) growth = MFMA_LEVEL_GROWTH;   // matrix-core launches: see the constant's comment
        if (k >= 256) growth = std::min<uint64_t>(growth, 2);   // simprint-sized k: candidate handling dominates, +10 % with short levels
        // a stretch `growth` times the rows seen so far brings ~growth * (rows at or under tau) candidates, and the
        // tie class at tau can make that 2.3x k (ratio of consecutive binomial tails): keep it inside the buffer
        while (growth > 2 && (uint64_t)k * growth * 5 / 2 > (uint64_t)cap * 9 / 10) growth /= 2;
        return growth;
    }
    int run_levels(Run& run) {
        const Job& j = run.j;
        const Segment& s = *j.seg;
        isk::ScanParams& sp = run.c.sp;
        const uint64_t tile_rows = (uint64_t)tile_rows_for((int)j.W);
        int rc;
        boot(run, false);
        // 2. levels: every level streams the NEXT stretch of rows [done, end) exactly once under the threshold of the
        //    rows before it, collecting its candidates and adding them to the running histogram (MODE_BOTH);
        //    pick_kernel then tightens the threshold to the k-th best so far and prunes the candidate list to
        //    it.  A level meets ~k * growth candidates per query, so the stretches grow geometrically (8x;
        //    64x when there are so few query groups that launch gaps outweigh candidate handling; less
        //    when k * growth would not fit the candidate buffer).  No row is read twice.
        const uint64_t growth = level_growth(j);
        uint64_t done = 0;                    // rows [0, done) are collected and in the histogram
        uint64_t reach = sample_rows(j, false);   // the threshold in force comes from rows [0, reach)
        for (;;) {
            uint64_t end = reach >= s.n / growth ? s.n : reach * growth;
            if (end < s.n) end = end / tile_rows * tile_rows;
            if (end <= done || end + tile_rows > s.n) end = s.n;
            const bool last = end == s.n;
            if (last) break;                  // the final stretch is the streaming pass below
            if (!run.hist_live) {
                HIPOK(hipMemsetAsync(h->d_ghist.p, 0, (size_t)nq_pad * isk::HB * sizeof(uint32_t), h->stream));
                run.hist_live = true;
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
        if ((rc = collect(run, collected_to))) return rc;

        // 4. exact select of the k best candidates per query (flags candidate-list overflow)
        launch_select(run.c.sl, nq);
        HIPOK(hipGetLastError());
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
        for (size_t ji = 0; ji < jobs.size(); ++ji)
            for (uint32_t q = 0; q < nq; ++q)
                if (flagged(ji, q) && (rc = fix_query(ji, q))) return rc;
        return 0;
    }
    int fix_query(size_t ji, uint32_t q) {
        const Job& j = jobs[ji];
        Segment& s = *j.seg;
        int rc;
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
            return 0;
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
            isk::with_key_words(t.key_words, [&](auto kw) { hipLaunchKernelGGL(isk::fb_keyhist_kernel<decltype(kw)::value>, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fb); });
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
        isk::with_key_words(t.key_words, [&](auto kw) { hipLaunchKernelGGL(isk::fb_collect_kernel<decltype(kw)::value>, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fb); });
        isk::SelectParams fsl = c.sl;
        fsl.cnt = h->d_cnt.p; fsl.cap = fb.cap; fsl.q_base = q;
        fsl.cand = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(h->d_misc2.p) - (uintptr_t)q * fsl.cap * 8);
        HIPOK(hipMemsetAsync(c.sl.overflow + q, 0, sizeof(uint32_t), h->stream));
        launch_select(fsl, 1);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(h->stream));
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
