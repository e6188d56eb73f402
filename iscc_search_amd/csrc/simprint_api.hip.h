// simprint_api.hip.h -- the four simprint entry points: a search whose lists stay on the device (ScoreSink) and the scoring of
// simprint_score.hip behind it, on the handle's SimprintScratch, staged through ScoreStaging (simprint_scratch.hip.h).
// Needs search_locked and ScoreSink of search_api.hip.h, ensure_freq_column of store.hip.h.
// What a ScoreSink (search_api.hip.h) does with a batch of the search: the approximate requests mark and compact it, a hard-boundary
// request keeps the lengths of its collision lists -- and prepares hits and offsets at once when the batch holds every lookup
hipError_t ScoreSink::queue_behind_select(uint32_t pos, uint32_t m, uint32_t k, const uint32_t* d_cnt, uint32_t* d_info, hipStream_t stream) const {
    const isksp::Buffers buf = sp.buffers();
    if (!exact) return isksp::queue_batch(buf, isksp::BatchArgs{pos, m, k, d_cnt, h_max, dup_limit, entries, d_info}, stream);
    const hipError_t e = hipMemcpyAsync(sp.cnt.p + pos, d_cnt, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess || !holds_every_lookup(pos, m)) return e;
    return isksp::exact_prepare(buf, d_cnt, sp.d_of_g.p, nd, ng, k, d_info, stream);
}
void ScoreSink::take(uint32_t pos, uint32_t m, uint32_t k, const uint32_t* p_cnt, const uint32_t* p_info) {
    if (!exact) {
        entries = p_info[0];
        unknown_any = unknown_any || p_info[1] != 0;
    } else if (holds_every_lookup(pos, m)) {
        entries = p_info[0];
        prepared = true;
    }
    for (uint32_t i = 0; i < m; ++i) max_count = std::max(max_count, std::min(p_cnt[i], k));
    if (q_count) for (uint32_t i = 0; i < m; ++i) q_count[pos + i] = std::min(p_cnt[i], k);
}

namespace {
// The match threshold on the integer distance, the table's frequency column and the similarity / IDF tables of one scoring call
// (isccsearch_simprint_score and _many); h->mu is held.
int simprint_setup(H* h, Table& t, Segment& s, double threshold, int64_t total_assets, uint32_t dup_limit, int& h_max) {
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
    if (h->sp.tab_bits != bits || h->sp.tab_dup != dup_limit || h->sp.tab_total != total_assets) {
        const size_t words = (size_t)bits + 1 + n_idf;
        if ((rc = h->sp.p_tab.ensure(words))) return rc;
        if ((rc = h->sp.tab.ensure(words))) return rc;
        HIPOK(hipStreamSynchronize(h->stream));      // (a previous upload may still be reading the staging block)
        double* tab = h->sp.p_tab.p;
        for (uint32_t d = 0; d <= bits; ++d) tab[d] = 1.0 - (double)d / (double)bits;
        auto idf = [&](uint32_t freq) { return total_assets <= 0 ? 0.0 : std::log(1.0 + (double)total_assets / (double)(1 + (uint64_t)freq)); };
        if (dup_limit) for (uint32_t f = 0; f <= dup_limit; ++f) tab[bits + 1 + f] = idf(f);
        else tab[bits + 1] = idf(1);
        HIPOK(hipMemcpyAsync(h->sp.tab.p, tab, words * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->sp.tab_bits = bits; h->sp.tab_dup = dup_limit; h->sp.tab_total = total_assets;
    }
    return 0;
}

// rare: a query simprint with k equal stored rows and k < dup_limit -- its document frequency needs the collision scan
int simprint_unknown_freq(H* h, uint32_t table, Table& t, uint32_t nq, const uint64_t* q_words, uint32_t dup_limit) {
    int rc;
    std::vector<uint32_t> unk(nq), fq(nq);
    HIPOK(hipMemcpyAsync(unk.data(), h->sp.unknown.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(fq.data(), h->sp.freq_q.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    std::vector<uint32_t> which;
    for (uint32_t q = 0; q < nq; ++q) if (unk[q]) which.push_back(q);
    std::vector<uint64_t> qw(which.size() * (size_t)t.max_words);
    for (size_t i = 0; i < which.size(); ++i) memcpy(&qw[i * t.max_words], q_words + (size_t)which[i] * t.max_words, (size_t)t.max_words * 8);
    std::vector<uint32_t> freq(which.size());
    if ((rc = search_locked(h, table, (uint32_t)which.size(), qw.data(), nullptr, dup_limit, 0, SearchOut::doc_freq(freq.data())))) return rc;
    for (size_t i = 0; i < which.size(); ++i) fq[which[i]] = freq[i];
    HIPOK(hipMemcpyAsync(h->sp.freq_q.p, fq.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));       // (fq leaves scope)
    return 0;
}

// The scoring of isccsearch_simprint_score and _many once their arguments are checked (out_info zeroed; request r = query simprints
// [req_offsets[r], req_offsets[r + 1]), at most MAX_QUERY_SIMPRINTS each): consecutive requests of at most MAX_QUERY_SIMPRINTS query
// simprints form a round, a request is never split.  A round is ONE search with the lists left on the device and one scoring: a round
// of one request takes queue_score's pipeline, a round of several queue_score_many's (which returns per request what queue_score would).
int simprint_score_rounds(H* h, uint32_t table, uint32_t n_req, const uint32_t* req_offsets, const uint64_t* q_words,
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
    SimprintScratch& sp = h->sp;
    std::vector<uint32_t>& qbeg = sp.h_qbeg;
    std::vector<uint32_t>& q_count = sp.h_qcount;
    for (uint32_t r0 = 0; r0 < n_req;) {
        const uint32_t base = req_offsets[r0];
        uint32_t r1 = r0 + 1;
        while (r1 < n_req && req_offsets[r1 + 1] - base <= isksp::MAX_QUERY_SIMPRINTS) ++r1;
        const uint32_t nq = req_offsets[r1] - base, nr = r1 - r0;
        const uint64_t* const qw = q_words + (size_t)base * t.max_words;
        if (nq == 0) { r0 = r1; continue; }
        h->stats.searches += 1;
        if ((rc = sp.for_search(nq, k))) return rc;
        q_count.assign(nq, 0);
        ScoreSink sink{sp};
        sink.h_max = h_max;
        sink.dup_limit = dup_limit;
        sink.q_count = q_count.data();
        if ((rc = search_locked(h, table, nq, qw, nullptr, k, max_hamming < 0 ? -1 : max_hamming, SearchOut::to_sink(&sink)))) return rc;
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
        if ((rc = nr == 1 ? sp.for_scoring(nq, entries) : sp.for_round(nq, entries, nr, cap))) return rc;
        isksp::Buffers buf = sp.buffers();
        // outputs in pinned memory, written by the emit kernels themselves
        const ScoreStaging st{nr, cap, out_chunks ? (size_t)std::min<uint64_t>((uint64_t)limit * nq, entries) : 0, W};
        if ((rc = sp.p_out.ensure(st.bytes()))) return rc;
        unsigned char* const po = sp.p_out.p;
        isksp::ScoreArgs sa{};
        sa.nq = nq; sa.k = k; sa.entries = entries; sa.limit = limit;
        sa.sim_tab = sp.tab.p; sa.idf_tab = sp.tab.p + bits + 1; sa.dup_limit = dup_limit;
        sa.freq_col = dup_limit ? s.freq : nullptr;
        set_cols(sa.col, s, s.W);
        sa.W = W;
        sa.out_info = st.info(po); sa.out_results = st.results(po); sa.out_chunks = st.chunks(po); sa.out_chunk_words = st.words(po);
        if (nr == 1) {
            HIPOK(isksp::queue_score(buf, sa, h->stream));
        } else {
            const isksp::ManyBuffers mb = sp.many_buffers();
            HIPOK(hipMemcpyAsync(mb.qbeg, qbeg.data(), (size_t)(nr + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            isksp::ScoreManyArgs ma{sa, nr, cap, words};
            HIPOK(isksp::queue_score_many(buf, mb, ma, h->stream));
        }
        HIPOK(hipStreamSynchronize(h->stream));       // (qbeg is read by the kernels until here)
        st.copy_out(po, limit, limit, req_offsets + r0, out_results + (size_t)r0 * limit, out_chunks, out_chunk_words, out_info + 4 * (size_t)r0);
        r0 = r1;
    }
    return 0;
}

// The hard-boundary search and scoring of isccsearch_simprint_exact and _exact_many once their arguments are checked (out_info zeroed;
// request r = the distinct simprints [distinct_offsets[r], distinct_offsets[r + 1]) and the given ones [given_offsets[r],
// given_offsets[r + 1]), whose `given` values are local to the request): consecutive requests of at most MAX_QUERY_SIMPRINTS given
// and at most as many distinct simprints form a round, a request is never split.  A round is ONE search at distance 0 over its
// distinct simprints with the collision lists left on the device, and one scoring: a round of one request takes queue_exact's
// pipeline, a round of several queue_exact_many's (which returns per request what queue_exact would).
int simprint_exact_rounds(H* h, uint32_t table, uint32_t n_req, const uint32_t* distinct_offsets, const uint64_t* q_words,
                          const uint32_t* given_offsets, const uint32_t* given, const uint32_t* queried,
                          uint32_t dup_limit, double threshold, uint32_t limit,
                          isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks, uint32_t* out_info) {
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
    const uint32_t k = std::min<uint32_t>(dup_limit, ISCCSEARCH_MAX_K);
    SimprintScratch& sp = h->sp;
    std::vector<uint32_t>& beg = sp.h_qbeg;         // {gbeg [nr + 1] | dbeg [nr + 1] | queried [nr]} of the round
    std::vector<uint32_t>& d_count = sp.h_qcount;   // length of every lookup's collision list
    std::vector<uint32_t>& d_of_g = sp.h_dofg;
    for (uint32_t r0 = 0; r0 < n_req;) {
        const uint32_t gbase = given_offsets[r0], dbase = distinct_offsets[r0];
        uint32_t r1 = r0 + 1;
        while (r1 < n_req && given_offsets[r1 + 1] - gbase <= isksp::MAX_QUERY_SIMPRINTS && distinct_offsets[r1 + 1] - dbase <= isksp::MAX_QUERY_SIMPRINTS) ++r1;
        const uint32_t ng = given_offsets[r1] - gbase, nd = distinct_offsets[r1] - dbase, nr = r1 - r0;
        if (ng == 0 || nd == 0) { r0 = r1; continue; }      // (given simprints index distinct ones: ng > 0 has nd > 0)
        h->stats.searches += 1;
        if ((rc = sp.for_exact_search(nd, ng, k))) return rc;
        // the round-global lookup of every given simprint, and where every request's given and distinct simprints begin
        beg.resize(3 * ((size_t)nr + 1));
        uint32_t* const gbeg = beg.data(), * const dbeg = gbeg + nr + 1, * const qd = dbeg + nr + 1;
        d_of_g.resize(ng);
        uint32_t words = 0;                // LDS words of the score kernel: those of the request with the most distinct simprints
        for (uint32_t r = 0; r < nr; ++r) {
            gbeg[r] = given_offsets[r0 + r] - gbase;
            dbeg[r] = distinct_offsets[r0 + r] - dbase;
            qd[r] = queried[r0 + r];
            for (uint32_t g = given_offsets[r0 + r]; g < given_offsets[r0 + r + 1]; ++g) d_of_g[g - gbase] = given[g] + dbeg[r];
            words = std::max(words, (distinct_offsets[r0 + r + 1] - distinct_offsets[r0 + r] + 63) / 64);
        }
        gbeg[nr] = ng; dbeg[nr] = nd; qd[nr] = 0;
        d_count.assign(nd, 0);
        ScoreSink sink{sp};
        sink.exact = true;
        sink.nd = nd; sink.ng = ng;
        sink.q_count = d_count.data();
        // (the lookup of every given simprint goes up first: when one batch holds all lookups, hits and offsets are prepared behind its
        //  select and the number of entries arrives with the batch's own synchronisation)
        HIPOK(hipMemcpyAsync(sp.d_of_g.p, d_of_g.data(), (size_t)ng * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));           // (d_of_g is rewritten by the next round)
        // every row equal to a query simprint, ascending key, at most dup_limit per simprint (lmdb_ops.py:197-210): the lists stay on the device
        if ((rc = search_locked(h, table, nd, q_words + (size_t)dbase * t.max_words, nullptr, k, 0, SearchOut::to_sink(&sink)))) return rc;
        for (uint32_t r = 0; r < nr; ++r) {
            uint32_t longest = 0;
            for (uint32_t d = dbeg[r]; d < dbeg[r + 1]; ++d) longest = std::max(longest, d_count[d]);
            out_info[4 * (size_t)(r0 + r) + 2] = longest;
        }
        uint32_t entries = sink.entries;
        if (!sink.prepared) {
            // several batches of lookups: hits per given simprint and their offsets now; the number of entries comes back with one small copy
            if ((rc = h->d_block.ensure(isksp::INFO_WORDS * sizeof(uint32_t)))) return rc;
            if ((rc = h->p_block.ensure(isksp::INFO_WORDS * sizeof(uint32_t)))) return rc;
            uint32_t* const d_info = reinterpret_cast<uint32_t*>(h->d_block.p);
            HIPOK(isksp::exact_prepare(sp.buffers(), sp.cnt.p, sp.d_of_g.p, nd, ng, k, d_info, h->stream));
            HIPOK(hipMemcpyAsync(h->p_block.p, d_info, isksp::INFO_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            HIPOK(hipStreamSynchronize(h->stream));
            entries = reinterpret_cast<const uint32_t*>(h->p_block.p)[0];
        }
        if (entries == 0) { r0 = r1; continue; }
        const uint32_t cap = nr == 1 ? limit : (uint32_t)std::min<uint64_t>((uint64_t)nr * limit, entries);
        if ((rc = nr == 1 ? sp.for_exact_scoring(entries) : sp.for_exact_round(entries, nr, cap))) return rc;
        isksp::Buffers buf = sp.buffers();
        const ScoreStaging st{nr, cap, out_chunks ? entries : 0, 0};
        if ((rc = sp.p_out.ensure(st.bytes()))) return rc;
        unsigned char* const po = sp.p_out.p;
        isksp::ExactArgs ea{};
        ea.nd = nd; ea.ng = ng; ea.k = k; ea.entries = entries; ea.limit = limit; ea.queried = qd[0];
        ea.d_of_g = sp.d_of_g.p; ea.threshold = threshold;
        ea.out_info = st.info(po); ea.out_results = st.results(po); ea.out_chunks = st.chunks(po);
        if (nr == 1) {
            HIPOK(isksp::queue_exact(buf, ea, h->stream));
        } else {
            const isksp::ManyBuffers mb = sp.many_buffers();
            HIPOK(hipMemcpyAsync(mb.qbeg, beg.data(), beg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            const isksp::ExactManyArgs ma{ea, nr, cap, words, mb.qbeg + nr + 1, mb.qbeg + 2 * ((size_t)nr + 1)};
            HIPOK(isksp::queue_exact_many(buf, mb, ma, h->stream));
        }
        HIPOK(hipStreamSynchronize(h->stream));       // (beg is read by the copy until here)
        st.copy_out(po, limit, k, given_offsets + r0, out_results + (size_t)r0 * limit, out_chunks, nullptr, out_info + 4 * (size_t)r0);
        r0 = r1;
    }
    return 0;
}

// what isccsearch_simprint_score and isccsearch_simprint_score_many check alike, and first
int check_score_args(const isccsearch_handle* h, uint32_t count, int32_t max_hamming, uint32_t dup_limit, uint32_t limit) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (int rc = check_count(count)) return rc;
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", max_hamming);
    if (dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u exceeds ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (limit < 1) return fail(-EINVAL, "limit must be >= 1");
    return 0;
}
}  // namespace

extern "C" {
// Search + asset scoring with the neighbour lists kept on the device (usearch_core.py:137-269); see include/isccsearch.h.
int isccsearch_simprint_score(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                              uint32_t count, int32_t max_hamming, double threshold, uint32_t limit,
                              int64_t total_assets, uint32_t dup_limit,
                              isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks,
                              uint64_t* out_chunk_words, uint32_t* out_info) {
    if (int rc = check_score_args(h, count, max_hamming, dup_limit, limit)) return rc;
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
    if (int rc = check_score_args(h, count, max_hamming, dup_limit, limit)) return rc;
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
    // (one request whose given simprints begin at 0: a round of one, queue_exact's pipeline)
    const uint32_t distinct_offsets[2] = {0, n_distinct}, given_offsets[2] = {0, n_given};
    return simprint_exact_rounds(h, table, 1, distinct_offsets, q_words, given_offsets, given, &queried, dup_limit, threshold, limit,
                                 out_results, out_chunks, out_info);
}

// Many hard-boundary requests against one table, each searched and scored on its own (lmdb_ops.py:169-301 per request); see include/isccsearch.h.
int isccsearch_simprint_exact_many(isccsearch_handle* h, uint32_t table, uint32_t n_req, const uint32_t* distinct_offsets, const uint64_t* q_words,
                                   const uint32_t* given_offsets, const uint32_t* given, const uint32_t* queried,
                                   uint32_t dup_limit, double threshold, uint32_t limit,
                                   isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks, uint32_t* out_info) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1) return fail(-EINVAL, "dup_limit must be >= 1");
    if (limit < 1) return fail(-EINVAL, "limit must be >= 1");
    if (n_req == 0) return 0;
    if (!out_info || !distinct_offsets || !given_offsets || !queried) return fail(-EINVAL, "NULL argument");
    memset(out_info, 0, (size_t)n_req * 4 * sizeof(uint32_t));
    for (uint32_t r = 0; r < n_req; ++r) {
        if (distinct_offsets[r + 1] < distinct_offsets[r]) return fail(-EINVAL, "distinct_offsets must not decrease (request %u)", r);
        if (given_offsets[r + 1] < given_offsets[r]) return fail(-EINVAL, "given_offsets must not decrease (request %u)", r);
    }
    for (uint32_t r = 0; r < n_req; ++r) {
        const uint32_t nd = distinct_offsets[r + 1] - distinct_offsets[r], ng = given_offsets[r + 1] - given_offsets[r];
        if (nd > isksp::MAX_QUERY_SIMPRINTS || ng > isksp::MAX_QUERY_SIMPRINTS)
            return fail(-E2BIG, "request %u: %u / %u query simprints exceed the %u one scoring call takes", r, nd, ng, isksp::MAX_QUERY_SIMPRINTS);
    }
    for (uint32_t r = 0; r < n_req; ++r) {
        const uint32_t ng = given_offsets[r + 1] - given_offsets[r];
        if (queried[r] < ng)
            return fail(-EINVAL, "request %u: queried (%u) counts every query simprint as given: it cannot be below its given simprints (%u)", r, queried[r], ng);
    }
    if (given_offsets[n_req] == given_offsets[0]) return 0;
    if (!q_words || !given || !out_results) return fail(-EINVAL, "NULL argument");
    for (uint32_t r = 0; r < n_req; ++r) {
        const uint32_t nd = distinct_offsets[r + 1] - distinct_offsets[r];
        for (uint32_t g = given_offsets[r]; g < given_offsets[r + 1]; ++g)
            if (given[g] >= nd) return fail(-EINVAL, "request %u: given[%u] = %u is no index into its %u distinct simprints", r, g, given[g], nd);
    }
    const uint32_t k = std::min<uint32_t>(dup_limit, ISCCSEARCH_MAX_K);
    if ((uint64_t)limit * n_req > 0xFFFFFFFFull)
        return fail(-E2BIG, "limit %u x %u requests exceeds the 32-bit result addressing", limit, n_req);
    if ((uint64_t)k * given_offsets[n_req] > 0xFFFFFFFFull)
        return fail(-E2BIG, "%u collisions x %u given simprints exceed the 32-bit chunk addressing", k, given_offsets[n_req]);
    if (!(threshold == threshold)) return fail(-EINVAL, "threshold is not a number");
    return simprint_exact_rounds(h, table, n_req, distinct_offsets, q_words, given_offsets, given, queried, dup_limit, threshold, limit,
                                 out_results, out_chunks, out_info);
}
}  // extern "C"
