// assets_api.hip.h -- isccsearch_match_assets.  Needs Batch and of isccsearch.hip, the tables of store.hip.h.
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
        if (c.deferred) { flag_total += flag_slots_for(m); pq_words += staged_words_for(m); }
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
            if (c.deferred) { c.flag_off = f - cnt_total; c.d_flags = h->d_am_cnt.p + f; f += flag_slots_for(c.units.size()); }
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
    if ((rc = wait_staged(h))) return rc;
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
        pq_off += staged_words_for(c.units.size());
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

    // (5) the caller's arrays.  The kernel writes a query's listed results only: past its count the staging area still holds what an
    // earlier call left there, and the caller gets zeros (types 0xFF), as the host path pads them
    memcpy(out_count, po + o_count, (size_t)nq * 4);
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t at = (size_t)q * limit, c = std::min<uint32_t>(out_count[q], limit), rest = limit - c;
        memcpy(out_keys + at, po + o_keys + at * 8, c * 8);
        memset(out_keys + at + c, 0, rest * 8);
        memcpy(out_scores + at, po + o_scores + at * 8, c * 8);
        memset(out_scores + at + c, 0, rest * 8);
        memcpy(out_types + at * n_types, po + o_types + at * n_types, c * n_types);
        memset(out_types + (at + c) * n_types, 0xFF, rest * n_types);
        memcpy(out_type_scores + at * n_types, po + o_types_sc + at * n_types * 8, c * n_types * 8);
        memset(out_type_scores + (at + c) * n_types, 0, rest * n_types * 8);
    }
    memcpy(out_unit_count, po + o_ucnt, (size_t)n_units * 4);
    return 0;
}
