// simprint_scratch.hip.h -- what a handle keeps for the simprint entry points of simprint_api.hip.h: the device buffers of
// simprint_score.hip's kernels with ONE place that sizes them per phase of a call and one that hands them to the kernels, and the
// layout of the pinned block the emit kernels write.  Needs DevBuf / PinBuf of isccsearch.hip (included inside its namespace).

// the first failure of b.ensure(n) over the buffers, or 0
template <typename... B>
int ensure_all(size_t n, B&... bufs) {
    int rc = 0;
    (void)((rc = bufs.ensure(n)) || ...);
    return rc;
}

struct SimprintScratch {
    // the neighbour lists of one request stay on the device with the segment row of every record; per record / per query simprint /
    // per entry what simprint_score.h's Buffers says
    DevBuf<isk::Record> rec;
    DevBuf<uint32_t> rows, nbest, offs, freq_q, unknown, entry[2], order[2], matches, n_assets;
    DevBuf<uint8_t> best;
    DevBuf<uint64_t> asset[2];
    DevBuf<double> score[2], ws, idf_q;
    DevBuf<unsigned char> temp;
    DevBuf<uint32_t> cnt, d_of_g;       // isccsearch_simprint_exact(_many): list lengths of every lookup, the lookup of every given simprint
    // a round of several requests (ManyBuffers): request keys / sort payloads per entry, per-request offsets and counts, chunks per result
    struct { DevBuf<uint32_t> req[2], idx[2], qbeg, n_assets, a_start, e_start, cnt, c_pos; } many;
    std::vector<uint32_t> h_qbeg, h_qcount;     // (host side of a round: kept, so that a scoring call allocates nothing here)
    std::vector<uint32_t> h_dofg;               // (... of a hard-boundary round: the round-global lookup of every given simprint)
    // the similarity / IDF tables on the device are those of (bits, total_assets, dup_limit):
    DevBuf<double> tab;
    PinBuf<double> p_tab;
    uint32_t tab_bits = 0, tab_dup = 0xFFFFFFFFu;
    int64_t tab_total = -1;
    PinBuf<unsigned char> p_out;        // the staging block (ScoreStaging)

    // -- sizing: one function per phase of a call --------------------------------------------------------------------------------
    // the search of a request of nq query simprints with k neighbours each, marked and compacted batch by batch
    int for_search(uint32_t nq, uint32_t k) {
        const size_t slots = (size_t)nq * k;
        int rc;
        if ((rc = ensure_all(slots, rec, rows, best, asset[0], entry[0], asset[1], entry[1]))) return rc;
        if ((rc = ensure_all(nq, nbest, offs, freq_q, unknown))) return rc;
        return n_assets.ensure(1);
    }
    // what weights and scores are written to, per sorted entry and per query simprint
    int for_scores(uint32_t nq, uint32_t entries) {
        const int rc = ensure_all(entries, score[0], order[0], score[1], order[1], matches, ws);
        return rc ? rc : idf_q.ensure(nq);
    }
    // its scoring, once the number of entries is known (queue_score)
    int for_scoring(uint32_t nq, uint32_t entries) {
        const int rc = for_scores(nq, entries);
        return rc ? rc : temp.ensure(isksp::sort_temp_bytes(entries));
    }
    // ... or that of a round of nr > 1 requests that writes at most `cap` results (queue_score_many)
    int for_round(uint32_t nq, uint32_t entries, uint32_t nr, uint32_t cap) {
        int rc;
        if ((rc = for_scores(nq, entries))) return rc;
        if ((rc = ensure_all(entries, many.req[0], many.idx[0], many.req[1], many.idx[1]))) return rc;
        if ((rc = ensure_all((size_t)nr + 1, many.qbeg, many.a_start, many.e_start))) return rc;
        if ((rc = many.n_assets.ensure(nr))) return rc;
        if ((rc = ensure_all(cap, many.cnt, many.c_pos))) return rc;
        return temp.ensure(isksp::many_temp_bytes(entries, cap));
    }
    // a hard-boundary request: the collision lists of nd distinct simprints, k rows each, and the ng simprints as given ...
    int for_exact_search(uint32_t nd, uint32_t ng, uint32_t k) {
        int rc;
        if ((rc = rec.ensure((size_t)nd * k))) return rc;
        if ((rc = ensure_all(nd, cnt, freq_q))) return rc;
        if ((rc = ensure_all(ng, d_of_g, nbest, unknown, offs))) return rc;
        return n_assets.ensure(1);
    }
    // ... and its scoring (queue_exact)
    int for_exact_scoring(uint32_t entries) {
        int rc;
        if ((rc = ensure_all(entries, asset[0], entry[0], asset[1], entry[1], score[0], order[0], score[1], order[1], matches))) return rc;
        return temp.ensure(isksp::sort_temp_bytes(entries));
    }

    // ... or that of a round of nr > 1 hard-boundary requests that writes at most `cap` results (queue_exact_many); many.qbeg holds
    // {gbeg [nr + 1] | dbeg [nr + 1] | queried [nr]}
    int for_exact_round(uint32_t entries, uint32_t nr, uint32_t cap) {
        int rc;
        if ((rc = ensure_all(entries, asset[0], entry[0], asset[1], entry[1], score[0], order[0], score[1], order[1], matches))) return rc;
        if ((rc = ensure_all(entries, many.req[0], many.idx[0], many.req[1], many.idx[1]))) return rc;
        if ((rc = many.qbeg.ensure(3 * ((size_t)nr + 1)))) return rc;
        if ((rc = ensure_all((size_t)nr + 1, many.a_start, many.e_start))) return rc;
        if ((rc = many.n_assets.ensure(nr))) return rc;
        if ((rc = ensure_all(cap, many.cnt, many.c_pos))) return rc;
        return temp.ensure(isksp::many_temp_bytes(entries, cap));
    }

    // -- the buffers as the kernels take them (after the sizing: a buffer that grew has moved) -----------------------------------
    isksp::Buffers buffers() const {
        isksp::Buffers b{};
        b.rec = reinterpret_cast<const isccsearch_record*>(rec.p);
        b.rows = rows.p; b.best = best.p; b.nbest = nbest.p; b.offs = offs.p;
        b.freq_q = freq_q.p; b.unknown = unknown.p; b.n_assets = n_assets.p;
        for (int i = 0; i < 2; ++i) { b.c_asset[i] = asset[i].p; b.c_entry[i] = entry[i].p; b.score[i] = score[i].p; b.order[i] = order[i].p; }
        b.matches = matches.p; b.ws = ws.p; b.idf_q = idf_q.p;
        b.temp = temp.p; b.temp_bytes = temp.n;
        return b;
    }
    isksp::ManyBuffers many_buffers() const {
        isksp::ManyBuffers mb{};
        for (int i = 0; i < 2; ++i) { mb.req[i] = many.req[i].p; mb.idx[i] = many.idx[i].p; }
        mb.qbeg = many.qbeg.p; mb.n_assets = many.n_assets.p; mb.a_start = many.a_start.p; mb.e_start = many.e_start.p;
        mb.cnt = many.cnt.p; mb.c_pos = many.c_pos.p;
        return mb;
    }
};

// The pinned block a scoring pipeline's emit kernel writes, compact, and the host reads after one synchronisation:
// {info [n_req][4] | results [cap] | chunks [chunk_cap] | chunk words [chunk_cap][W]}; chunk_cap == 0: the caller wants no chunks.
// Request r's results follow those of the requests before it, its chunks likewise; info[4 r ..] = {results, assets matched, -, chunks}.
struct ScoreStaging {
    size_t n_req, cap, chunk_cap, W;
    constexpr size_t results_off() const { return (n_req * 4 * sizeof(uint32_t) + 15) / 16 * 16; }
    constexpr size_t chunks_off() const { return results_off() + cap * sizeof(isccsearch_simprint_result); }
    constexpr size_t words_off() const { return chunks_off() + chunk_cap * sizeof(isccsearch_simprint_chunk); }
    constexpr size_t bytes() const { return words_off() + chunk_cap * W * sizeof(uint64_t); }
    uint32_t* info(unsigned char* base) const { return reinterpret_cast<uint32_t*>(base); }
    isccsearch_simprint_result* results(unsigned char* base) const { return reinterpret_cast<isccsearch_simprint_result*>(base + results_off()); }
    // (nullptr tells the emit kernels that no chunks are wanted)
    isccsearch_simprint_chunk* chunks(unsigned char* base) const { return chunk_cap ? reinterpret_cast<isccsearch_simprint_chunk*>(base + chunks_off()) : nullptr; }
    uint64_t* words(unsigned char* base) const { return chunk_cap && W ? reinterpret_cast<uint64_t*>(base + words_off()) : nullptr; }
    // Into the caller's regions: request r's results at r x limit, its chunks (and their words) at chunk_stride x first_query[r] (the
    // most chunks a query simprint can have: `limit` of an approximate request, k of a hard-boundary one), its counts in
    // out_info[4 r ..] (word 2, the longest list, is the search's and stays)
    void copy_out(unsigned char* base, uint32_t limit, uint32_t chunk_stride, const uint32_t* first_query, isccsearch_simprint_result* out_results,
                  isccsearch_simprint_chunk* out_chunks, uint64_t* out_chunk_words, uint32_t* out_info) const {
        const uint32_t* in = info(base);
        size_t res_at = 0, chunk_at = 0;
        for (size_t r = 0; r < n_req; ++r) {
            const uint32_t n = in[4 * r], c = in[4 * r + 3];
            out_info[4 * r] = n; out_info[4 * r + 1] = in[4 * r + 1]; out_info[4 * r + 3] = c;
            memcpy(out_results + r * limit, results(base) + res_at, (size_t)n * sizeof(isccsearch_simprint_result));
            if (chunk_cap && c) {
                const size_t dst = (size_t)chunk_stride * first_query[r];
                memcpy(out_chunks + dst, chunks(base) + chunk_at, (size_t)c * sizeof(isccsearch_simprint_chunk));
                if (W) memcpy(out_chunk_words + dst * W, words(base) + chunk_at * W, (size_t)c * W * sizeof(uint64_t));
            }
            res_at += n;
            chunk_at += c;
        }
    }
};
static_assert(sizeof(isccsearch_simprint_result) == 24 && sizeof(isccsearch_simprint_chunk) == 24, "the records of include/isccsearch.h");
static_assert(ScoreStaging{1, 10, 0, 0}.results_off() == 16 && ScoreStaging{1, 10, 0, 0}.bytes() == 16 + 10 * 24, "one request, no chunks");
static_assert(ScoreStaging{1, 2, 7, 0}.words_off() == 16 + 2 * 24 + 7 * 24 && ScoreStaging{1, 2, 7, 0}.bytes() == ScoreStaging{1, 2, 7, 0}.words_off(),
              "a hard-boundary request: collisions carry no code words");
static_assert(ScoreStaging{3, 5, 7, 2}.results_off() == 48 && ScoreStaging{3, 5, 7, 2}.chunks_off() == 48 + 5 * 24 &&
              ScoreStaging{3, 5, 7, 2}.words_off() == 48 + 5 * 24 + 7 * 24 && ScoreStaging{3, 5, 7, 2}.bytes() == 48 + 5 * 24 + 7 * 24 + 7 * 2 * 8, "a round of three");
