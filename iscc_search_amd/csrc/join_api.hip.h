// join_api.hip.h -- isccsearch_join_within and isccsearch_join_between: the self-join of a table and the cross join of two
// tables by the XOR + popcount kernel of join.hip.h or, for launches over enough rows, its matrix-core form (mfma_join_kernel.hip.h);
// and isccsearch_join_components: the self-join's launches in their LINK form, whose pairs are united in a union-find array
// (unionfind.hip.h) instead of written; and isccsearch_join_degrees: those launches in their DEGREE form, which leave a count per listed
// row; and isccsearch_join_within_live: the self-join's pairs among the listed rows (the LIVE form); and isccsearch_join_overlaps:
// the self-join of a simprint table in the launches' OVERLAP form, whose directed hits overlap.hip sorts and reduces to one record per ordered pair of assets; and isccsearch_join_segments: the same
// call, whose chunk pairs segments.hip turns into aligned runs before they are reduced; and isccsearch_join_overlaps_between: the
// cross join of two simprint tables in the same OVERLAP form, with a label space per table; and isccsearch_join_segments_between:
// that call with the same stage of segments.hip over the two tables.
// Needs the store of isccsearch.hip (Segment, Table; get_table of store.hip.h) and its scratch buffers.
namespace {
// one launch of the join kernel (join.hip.h) in the form (form, cross); false: that form is not instantiated
bool launch_join(isk::JoinForm form, bool cross, uint32_t W, const isk::JoinParams& jp, bool mask, uint64_t blocks, hipStream_t stream) {
    return isk::with_join_form(form, cross, [&](auto f) { isk::with_words((int)W, [&](auto w) {
        constexpr int WORDS = decltype(w)::value;
        constexpr isk::JoinForm F = decltype(f)::form;
        constexpr bool CROSS = decltype(f)::cross;
        if (mask) hipLaunchKernelGGL((isk::join_scan_kernel<WORDS, true, F, CROSS>), dim3((uint32_t)blocks), dim3(isk::BLOCK), 0, stream, jp);
        else hipLaunchKernelGGL((isk::join_scan_kernel<WORDS, false, F, CROSS>), dim3((uint32_t)blocks), dim3(isk::BLOCK), 0, stream, jp);
    }); });
}
constexpr uint32_t join_rows_per_block(uint32_t W) {
    return W == 1 ? isk::join_rows_per_block<1>() : W == 2 ? isk::join_rows_per_block<2>() : W == 3 ? isk::join_rows_per_block<3>() : isk::join_rows_per_block<4>();
}
// the grid of the one-thread-per-row kernels beside the joins (they stride over what a grid of 2^16 blocks leaves)
uint32_t row_blocks(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + isk::BLOCK - 1) / isk::BLOCK, 1u << 16); }
// keys[0 .. n) strictly ascending, or the refusal that names the argument (not_ascending: the test of one entry, for a caller whose
// pass over the keys checks more than this)
inline bool not_ascending(const uint64_t* keys, uint64_t i) { return i && keys[i] <= keys[i - 1]; }
int fail_not_ascending(const char* name, uint64_t i) {
    return fail(-EINVAL, "%s must be strictly ascending: %s[%llu] <= %s[%llu]", name, name, (unsigned long long)i, name, (unsigned long long)(i - 1));
}
int check_ascending(const char* name, const uint64_t* keys, uint64_t n) {
    for (uint64_t i = 1; i < n; ++i)
        if (not_ascending(keys, i)) return fail_not_ascending(name, i);
    return 0;
}

// One call's launches: one per pair of segments, all appending to one output.  What only the emit path reads goes to the
// device as one array of descriptors.
struct JoinPlan {
    // mfma: the launch takes mfma_join_kernel (mp, chunks of `groups` * 32 held rows), else join_scan_kernel (jp, blocks)
    struct Launch { isk::JoinParams jp; uint32_t W; bool mask; uint64_t blocks; bool mfma; isk::MfmaJoinParams mp; uint32_t groups; uint64_t chunks; };
    std::vector<Launch> launches;
    std::vector<isk::JoinEmit> emits;
    isk::JoinForm form = isk::JoinForm::PAIRS;     // the form of either kernel, with `cross`: join.hip.h
    bool cross = false;
    uint32_t KW = 1;
    uint64_t capacity = 0, cap_alloc = 1;
    // what the form's emit path needs besides the rows' labels (join_add): set by the caller after join_begin
    uint32_t* parent = nullptr;                    // LINK: the union-find array
    uint4* out_hits = nullptr;                     // OVERLAP: [2 * capacity]
    bool skip_same_key = false;                    // OVERLAP, cross
    uint32_t* degree = nullptr;                    // DEGREE: a counter per label
};

int join_check_args(isccsearch_handle* h, const int16_t* max_hamming, uint64_t capacity, uint64_t* out_keys_a, uint64_t* out_keys_b,
                    uint32_t* out_hamming, uint16_t* out_prefix_bits, uint64_t* out_total) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!max_hamming || !out_total) return fail(-EINVAL, "NULL argument");
    *out_total = 0;
    if (capacity && (!out_keys_a || !out_keys_b || !out_hamming || !out_prefix_bits))
        return fail(-EINVAL, "NULL output array with capacity %llu", (unsigned long long)capacity);
    return 0;
}

// The plan of one call in the form (form, cross) and the call's counters, zeroed ([0] is the pair counter every launch adds to).  The
// output buffers of PAIRS (and LIVE, which writes what PAIRS writes) are sized here; LINK, OVERLAP and DEGREE write none of them.
int join_begin(isccsearch_handle* h, JoinPlan& plan, isk::JoinForm form, bool cross, uint32_t KW, uint64_t capacity, uint32_t n_counters = 1) {
    plan.form = form;
    plan.cross = cross;
    plan.KW = KW;
    plan.capacity = capacity;
    plan.cap_alloc = std::max<uint64_t>(capacity, 1);
    int rc;
    if (form == isk::JoinForm::PAIRS || form == isk::JoinForm::LIVE) {
        if ((rc = h->d_join_keys.ensure(plan.cap_alloc * 2 * KW))) return rc;
        if ((rc = h->d_join_ham.ensure(plan.cap_alloc))) return rc;
        if ((rc = h->d_join_pb.ensure(plan.cap_alloc))) return rc;
    }
    if ((rc = h->d_join_total.ensure(n_counters))) return rc;
    HIPOK(hipMemsetAsync(h->d_join_total.p, 0, n_counters * 8, h->stream));
    return 0;
}

// One launch: segment A (one block per TQ rows, the rows in SGPRs) against segment B (streamed by every block) over a common
// prefix of pbytes bytes under tau.  `same`: A and B are one segment (the self-join keeps row_a < row_b).  `sgpr_side_is_b`:
// a cross join whose segment A belongs to the call's table_b.  labels_a / labels_b: a label per row of A / B, for every form but PAIRS.
// On the matrix cores (options mfma, join_mfma; both segments of at least join_mfma_min_rows rows) segment A is the HELD side --
// chunks of its rows in LDS, what the SGPRs are to join_scan_kernel -- and B is streamed: the same roles, the same JoinEmit.
int join_add(isccsearch_handle* h, JoinPlan& plan, Segment& A, Segment& B, uint32_t pbytes, int tau, bool same, bool sgpr_side_is_b,
             const uint32_t* labels_a = nullptr, const uint32_t* labels_b = nullptr) {
    const uint32_t W = (pbytes + 7) / 8;
    JoinPlan::Launch L{};
    set_cols(L.jp.col_a, A, W);
    set_cols(L.jp.col_b, B, W);
    L.jp.n_a = A.n; L.jp.n_b = B.n;
    L.jp.mask = mask_for(pbytes);
    L.jp.tau = (uint32_t)std::min<int>(tau, 8 * ISCCSEARCH_MAX_BYTES);
    L.jp.same = same ? 1u : 0u;
    // the fields the plan's form reads (JoinEmit, join.hip.h); the others stay null
    isk::JoinEmit e{};
    e.n_a = A.n;
    e.capacity = plan.capacity;
    e.total = reinterpret_cast<unsigned long long*>(h->d_join_total.p);
    switch (plan.form) {
        case isk::JoinForm::LIVE:
            e.labels_a = labels_a; e.labels_b = labels_b;
            [[fallthrough]];
        case isk::JoinForm::PAIRS:
            e.keys_a = A.keys; e.keys_b = B.keys;
            e.out_keys_a = h->d_join_keys.p;
            e.out_keys_b = h->d_join_keys.p + plan.cap_alloc * plan.KW;
            e.out_hamming = h->d_join_ham.p;
            e.out_prefix_bits = h->d_join_pb.p;
            e.prefix_bits = 8 * pbytes;
            e.kw = plan.KW;
            e.sgpr_side_is_b = sgpr_side_is_b ? 1u : 0u;
            break;
        case isk::JoinForm::LINK:
            e.labels_a = labels_a; e.labels_b = labels_b;
            e.parent = plan.parent;
            break;
        case isk::JoinForm::OVERLAP:
            e.labels_a = labels_a; e.labels_b = labels_b;
            e.out_hits = plan.out_hits;
            e.keys_a = A.keys; e.keys_b = B.keys;      // (skip_same_key compares the rows' asset keys)
            e.skip_same_key = plan.skip_same_key ? 1u : 0u;
            break;
        case isk::JoinForm::DEGREE:
            e.labels_a = labels_a; e.labels_b = labels_b;
            e.degree = plan.degree;
            break;
    }
    // within one segment the last row pairs with no later one
    const uint64_t a_rows = same ? A.n - 1 : A.n;
    L.W = W;
    L.mask = pbytes % 8 != 0;
    L.blocks = (a_rows + join_rows_per_block(W) - 1) / join_rows_per_block(W);
    if (L.blocks >= (1ull << 31) || B.n >= (1ull << 40))
        return fail(-E2BIG, "segments of %llu x %llu rows exceed the join kernel's grid", (unsigned long long)A.n, (unsigned long long)B.n);
    const uint64_t min_rows = (uint64_t)h->opt.join_mfma_min_rows;
    L.mfma = h->opt.mfma && h->opt.join_mfma && A.n >= min_rows && B.n >= min_rows;
    if (L.mfma) {
        set_cols(L.mp.col_q, A, W);
        set_cols(L.mp.col_s, B, W);
        L.mp.n_q = A.n; L.mp.n_s = B.n;
        L.mp.mask_lo = (uint32_t)L.jp.mask; L.mp.mask_hi = (uint32_t)(L.jp.mask >> 32);
        L.mp.tau = L.jp.tau;
        L.mp.same = L.jp.same;
        L.groups = isk::mfma_join_groups_per_chunk((int)W, A.n, plan.form);
        L.chunks = (A.n + L.groups * 32 - 1) / (L.groups * 32);
    }
    plan.launches.push_back(L);
    plan.emits.push_back(e);
    return 0;
}

// The launches of a table's self-join: add(a_len, b_len, pbytes, same) for every pair of non-empty segments la <= lb that
// max_hamming admits (the pair compares pbytes = la bytes under max_hamming[la]; `same`: la == lb, which takes 2 rows).  Side A
// (a_len: one block per TQ rows, or held in LDS chunk by chunk) is the segment with more rows; side B is streamed by every block.
template <typename Add> int join_self_pairs(Table& t, const int16_t* max_hamming, Add&& add) {
    for (uint32_t la = 1; la <= ISCCSEARCH_MAX_BYTES; ++la) {
        if (!t.seg[la].n || max_hamming[la] < 0) continue;
        for (uint32_t lb = la; lb <= ISCCSEARCH_MAX_BYTES; ++lb) {
            const bool same = la == lb;
            if (!t.seg[lb].n || (same && t.seg[la].n < 2)) continue;
            const uint32_t a_len = t.seg[lb].n > t.seg[la].n ? lb : la, b_len = a_len == la ? lb : la;
            if (int rc = add(a_len, b_len, la, same)) return rc;
        }
    }
    return 0;
}

// A label per row of a table of 64-bit keys, segment by segment, queued on the handle's stream: live_keys (strictly ascending, checked by
// the caller) and their labels go to the device, label_rows_kernel runs once per segment (the host never sees the table's keys), and
// row_labels[l] names the labels of segment l in d_join_row_labels.  live_labels NULL: the label of a key is its index in live_keys.
int join_label_rows(isccsearch_handle* h, Table& t, uint64_t n_live, const uint64_t* live_keys, const uint32_t* live_labels,
                    uint32_t* (&row_labels)[ISCCSEARCH_MAX_BYTES + 1]) {
    int rc;
    if ((rc = h->d_join_live_keys.ensure(std::max<uint64_t>(n_live, 1)))) return rc;
    if (live_labels && (rc = h->d_join_live_labels.ensure(std::max<uint64_t>(n_live, 1)))) return rc;
    uint64_t all_rows = 0;
    for (uint32_t l = 1; l <= ISCCSEARCH_MAX_BYTES; ++l) all_rows += t.seg[l].n;
    if ((rc = h->d_join_row_labels.ensure(std::max<uint64_t>(all_rows, 1)))) return rc;
    if (n_live) {
        HIPOK(hipMemcpyAsync(h->d_join_live_keys.p, live_keys, n_live * 8, hipMemcpyHostToDevice, h->stream));
        if (live_labels) HIPOK(hipMemcpyAsync(h->d_join_live_labels.p, live_labels, n_live * 4, hipMemcpyHostToDevice, h->stream));
    }
    uint64_t rows = 0;
    for (uint32_t l = 1; l <= ISCCSEARCH_MAX_BYTES; ++l) {
        const Segment& s = t.seg[l];
        row_labels[l] = nullptr;
        if (!s.n) continue;
        row_labels[l] = h->d_join_row_labels.p + rows;
        rows += s.n;
        isk::LabelParams lp{s.keys, h->d_join_live_keys.p, live_labels ? h->d_join_live_labels.p : nullptr, row_labels[l], s.n, n_live};
        hipLaunchKernelGGL(isk::label_rows_kernel, dim3(row_blocks(s.n)), dim3(isk::BLOCK), 0, h->stream, lp);
        HIPOK(hipGetLastError());
    }
    return 0;
}

// The launches of one call, in order on the handle's stream.
int join_run(isccsearch_handle* h, JoinPlan& plan) {
    if (!plan.launches.empty()) {
        int rc;
        if ((rc = h->d_join_emit.ensure(plan.emits.size()))) return rc;
        HIPOK(hipMemcpyAsync(h->d_join_emit.p, plan.emits.data(), plan.emits.size() * sizeof(isk::JoinEmit), hipMemcpyHostToDevice, h->stream));
        for (size_t i = 0; i < plan.launches.size(); ++i) {
            JoinPlan::Launch& L = plan.launches[i];
            L.jp.e = L.mp.e = h->d_join_emit.p + i;
            if (L.mfma) {
                // grid.y is 16 bits: a segment of more chunks than one launch takes goes in several, each from its chunk_base
                const uint32_t blocks_x = isk::mfma_join_blocks_x(L.mp.n_s);
                for (uint64_t c = 0; c < L.chunks; c += isk::MFMA_JOIN_MAX_CHUNKS) {
                    L.mp.chunk_base = c;
                    const uint32_t chunks = (uint32_t)std::min<uint64_t>(L.chunks - c, isk::MFMA_JOIN_MAX_CHUNKS);
                    const int lrc = isk::launch_mfma_join((int)L.W, plan.form, plan.cross, blocks_x, chunks, L.groups, h->stream, L.mp);
                    if (lrc) return fail(-EINVAL, "the matrix-core join does not take chunks of %u groups of %u words", L.groups, L.W);
                    HIPOK(hipGetLastError());
                    h->stats.join_launches += 1;
                    h->stats.join_mfma_launches += 1;
                }
                continue;
            }
            if (!launch_join(plan.form, plan.cross, L.W, L.jp, L.mask, L.blocks, h->stream))
                return fail(-EINVAL, "the join kernel has no form %d%s", (int)plan.form, plan.cross ? " over two tables" : "");
            HIPOK(hipGetLastError());
            h->stats.join_launches += 1;
        }
    }
    return 0;
}

// The call's one synchronisation: the total read back behind everything the call put on the stream.
int join_total(isccsearch_handle* h, uint64_t* out_total) {
    uint64_t total = 0;
    HIPOK(hipMemcpyAsync(&total, h->d_join_total.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    *out_total = total;
    return 0;
}

// The shared tail of the two pair joins: the launches, the total read back, the pairs copied to the host and sorted by (key_a, key_b).
int join_finish(isccsearch_handle* h, JoinPlan& plan, uint64_t* out_keys_a, uint64_t* out_keys_b, uint32_t* out_hamming,
                uint16_t* out_prefix_bits, uint64_t* out_total) {
    const uint32_t KW = plan.KW;
    const uint64_t capacity = plan.capacity, cap_alloc = plan.cap_alloc;
    int rc;
    if ((rc = join_run(h, plan))) return rc;
    if ((rc = join_total(h, out_total))) return rc;
    const uint64_t total = *out_total;
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
}  // namespace

// One join launch per pair of segments (join_scan_kernel of join.hip.h or mfma_join_kernel, see join_add), all appending to one
// output; the pairs are sorted on the host.
extern "C" int isccsearch_join_within(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t capacity,
                           uint64_t* out_keys_a, uint64_t* out_keys_b, uint32_t* out_hamming, uint16_t* out_prefix_bits,
                           uint64_t* out_total) {
    int rc = join_check_args(h, max_hamming, capacity, out_keys_a, out_keys_b, out_hamming, out_prefix_bits, out_total);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    if ((rc = get_table(h, table, tp))) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    JoinPlan plan;
    if ((rc = join_begin(h, plan, isk::JoinForm::PAIRS, false, (uint32_t)t.key_words, capacity))) return rc;
    rc = join_self_pairs(t, max_hamming, [&](uint32_t a_len, uint32_t b_len, uint32_t pbytes, bool same) {
        return join_add(h, plan, t.seg[a_len], t.seg[b_len], pbytes, max_hamming[pbytes], same, false);
    });
    if (rc) return rc;
    return join_finish(h, plan, out_keys_a, out_keys_b, out_hamming, out_prefix_bits, out_total);
}

// One cross-join launch per pair of non-empty segments (la of table_a, lb of table_b), in either order of
// lengths: the pair compares min(la, lb) bytes.  Both tables live on this handle, so one lock covers the call.
extern "C" int isccsearch_join_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b, const int16_t* max_hamming,
                            uint64_t capacity, uint64_t* out_keys_a, uint64_t* out_keys_b, uint32_t* out_hamming,
                            uint16_t* out_prefix_bits, uint64_t* out_total) {
    int rc = join_check_args(h, max_hamming, capacity, out_keys_a, out_keys_b, out_hamming, out_prefix_bits, out_total);
    if (rc) return rc;
    if (table_a == table_b) return fail(-EINVAL, "join_between needs two tables (table %u given twice): isccsearch_join_within joins a table with itself", table_a);
    std::lock_guard<std::mutex> lk(h->mu);
    Table *ta, *tb;
    if ((rc = get_table(h, table_a, ta))) return rc;
    if ((rc = get_table(h, table_b, tb))) return rc;
    if (ta->metric != tb->metric) return fail(-EINVAL, "tables %u and %u differ in metric (%d, %d)", table_a, table_b, ta->metric, tb->metric);
    if (ta->key_words != tb->key_words)
        return fail(-EINVAL, "tables %u and %u differ in key_words (%d, %d)", table_a, table_b, ta->key_words, tb->key_words);
    if (ta->metric == ISCCSEARCH_METRIC_HAMMING && ta->max_bytes != tb->max_bytes)
        return fail(-EINVAL, "Hamming tables %u and %u hold codes of different lengths (%d, %d bytes)", table_a, table_b, ta->max_bytes, tb->max_bytes);
    HIPOK(hipSetDevice(h->device));
    JoinPlan plan;
    if ((rc = join_begin(h, plan, isk::JoinForm::PAIRS, true, (uint32_t)ta->key_words, capacity))) return rc;
    for (uint32_t la = 1; la <= ISCCSEARCH_MAX_BYTES; ++la) {
        if (!ta->seg[la].n) continue;
        for (uint32_t lb = 1; lb <= ISCCSEARCH_MAX_BYTES; ++lb) {
            const uint32_t p = std::min(la, lb);
            if (!tb->seg[lb].n || max_hamming[p] < 0) continue;
            // as in the self-join the segment with more rows goes into SGPRs (on the matrix cores: is held in LDS): that may be table B's
            const bool b_in_sgprs = tb->seg[lb].n > ta->seg[la].n;
            Segment& A = b_in_sgprs ? tb->seg[lb] : ta->seg[la];
            Segment& B = b_in_sgprs ? ta->seg[la] : tb->seg[lb];
            if ((rc = join_add(h, plan, A, B, p, max_hamming[p], false, b_in_sgprs))) return rc;
        }
    }
    return join_finish(h, plan, out_keys_a, out_keys_b, out_hamming, out_prefix_bits, out_total);
}

// The launches of isccsearch_join_within in their LINK form between label_rows_kernel (one per segment: the host never sees the table's keys) and flatten_kernel, all on one stream; then
// `parent` and the links come back behind one synchronisation.  Everything the device code relies on -- labels < n_labels,
// parent[i] <= i -- is checked on the host before anything is launched.
extern "C" int isccsearch_join_components(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t n_live,
                               const uint64_t* live_keys, const uint32_t* live_labels, uint32_t n_labels, uint32_t* parent,
                               uint64_t* out_links) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!max_hamming || !parent || !out_links || (n_live && (!live_keys || !live_labels))) return fail(-EINVAL, "NULL argument");
    *out_links = 0;
    if (n_labels == 0 || n_labels == isk::UF_NONE) return fail(-EINVAL, "n_labels must be in 1 .. 2^32 - 2, got %u", n_labels);
    for (uint64_t i = 0; i < n_live; ++i) {            // (one pass over both arrays: they can be millions of entries)
        if (not_ascending(live_keys, i)) return fail_not_ascending("live_keys", i);
        if (live_labels[i] >= n_labels)
            return fail(-EINVAL, "live_labels[%llu] = %u is not below n_labels = %u", (unsigned long long)i, live_labels[i], n_labels);
    }
    for (uint32_t i = 0; i < n_labels; ++i)
        if (parent[i] > i) return fail(-EINVAL, "parent[%u] = %u is above its index: the input forest needs parent[i] <= i", i, parent[i]);
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc;
    if ((rc = get_table(h, table, tp))) return rc;
    Table& t = *tp;
    if (t.key_words != 1) return fail(-EINVAL, "join_components needs a table of 64-bit keys (key_words 1), table %u has key_words %d", table, t.key_words);
    HIPOK(hipSetDevice(h->device));
    JoinPlan plan;
    if ((rc = join_begin(h, plan, isk::JoinForm::LINK, false, 1, 0))) return rc;
    if ((rc = h->d_join_parent.ensure(n_labels))) return rc;
    HIPOK(hipMemcpyAsync(h->d_join_parent.p, parent, (size_t)n_labels * 4, hipMemcpyHostToDevice, h->stream));
    // a label per row, segment by segment
    uint32_t* row_labels[ISCCSEARCH_MAX_BYTES + 1] = {};
    if ((rc = join_label_rows(h, t, n_live, live_keys, live_labels, row_labels))) return rc;
    // the launches of isccsearch_join_within
    plan.parent = h->d_join_parent.p;
    rc = join_self_pairs(t, max_hamming, [&](uint32_t a_len, uint32_t b_len, uint32_t pbytes, bool same) {
        return join_add(h, plan, t.seg[a_len], t.seg[b_len], pbytes, max_hamming[pbytes], same, false, row_labels[a_len], row_labels[b_len]);
    });
    if (rc) return rc;
    if ((rc = join_run(h, plan))) return rc;
    hipLaunchKernelGGL(isk::flatten_kernel, dim3(row_blocks(n_labels)), dim3(isk::BLOCK), 0, h->stream, h->d_join_parent.p, n_labels);
    HIPOK(hipGetLastError());
    // the array goes to a copy first: `parent` changes only once the whole call has succeeded
    std::vector<uint32_t> flat(n_labels);
    HIPOK(hipMemcpyAsync(flat.data(), h->d_join_parent.p, (size_t)n_labels * 4, hipMemcpyDeviceToHost, h->stream));
    if ((rc = join_total(h, out_links))) return rc;
    memcpy(parent, flat.data(), (size_t)n_labels * 4);
    return 0;
}

// isccsearch_join_degrees and isccsearch_join_within_live: the launches of isccsearch_join_within over the rows whose keys are listed, the
// label of a row being the index of its key in live_keys (join_label_rows without a label array).
namespace {
// what the two calls check alike, on the host, before anything is launched and before any output is touched; `t`: the table, locked
int join_live_check(isccsearch_handle* h, const char* name, uint32_t table, uint64_t n_live, const uint64_t* live_keys, Table*& t) {
    if (n_live >= isk::UF_NONE)
        return fail(-EINVAL, "n_live must be below 2^32 - 1 (the value that means \"no label\"), got %llu", (unsigned long long)n_live);
    if (int rc = check_ascending("live_keys", live_keys, n_live)) return rc;
    if (int rc = get_table(h, table, t)) return rc;
    if (t->key_words != 1) return fail(-EINVAL, "%s needs a table of 64-bit keys (key_words 1), table %u has key_words %d", name, table, t->key_words);
    return 0;
}
uint64_t table_rows(const Table& t) {
    uint64_t rows = 0;
    for (uint32_t l = 1; l <= ISCCSEARCH_MAX_BYTES; ++l) rows += t.seg[l].n;
    return rows;
}
}  // namespace

// The launches of isccsearch_join_within in their DEGREE form between label_rows_kernel and the copies, all on one stream: a counter per
// listed key (zeroed) and the links come back behind one synchronisation.
extern "C" int isccsearch_join_degrees(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t n_live, const uint64_t* live_keys,
                            uint32_t* out_degree, uint64_t* out_links) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!max_hamming || !out_links || (n_live && (!live_keys || !out_degree))) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc;
    if ((rc = join_live_check(h, "join_degrees", table, n_live, live_keys, tp))) return rc;
    Table& t = *tp;
    if (n_live < 2 || table_rows(t) < 2) {            // no pair of listed rows: nothing is launched
        if (n_live) memset(out_degree, 0, (size_t)n_live * 4);
        *out_links = 0;
        return 0;
    }
    HIPOK(hipSetDevice(h->device));
    JoinPlan plan;
    if ((rc = join_begin(h, plan, isk::JoinForm::DEGREE, false, 1, 0))) return rc;
    if ((rc = h->d_join_degree.ensure(n_live))) return rc;
    HIPOK(hipMemsetAsync(h->d_join_degree.p, 0, (size_t)n_live * 4, h->stream));
    uint32_t* row_labels[ISCCSEARCH_MAX_BYTES + 1] = {};
    if ((rc = join_label_rows(h, t, n_live, live_keys, nullptr, row_labels))) return rc;
    plan.degree = h->d_join_degree.p;
    rc = join_self_pairs(t, max_hamming, [&](uint32_t a_len, uint32_t b_len, uint32_t pbytes, bool same) {
        return join_add(h, plan, t.seg[a_len], t.seg[b_len], pbytes, max_hamming[pbytes], same, false, row_labels[a_len], row_labels[b_len]);
    });
    if (rc) return rc;
    if ((rc = join_run(h, plan))) return rc;
    // the counters go to a copy first: the outputs change only once the whole call has succeeded
    std::vector<uint32_t> degree(n_live);
    uint64_t links = 0;
    HIPOK(hipMemcpyAsync(degree.data(), h->d_join_degree.p, (size_t)n_live * 4, hipMemcpyDeviceToHost, h->stream));
    if ((rc = join_total(h, &links))) return rc;
    memcpy(out_degree, degree.data(), (size_t)n_live * 4);
    *out_links = links;
    return 0;
}

// The launches of isccsearch_join_within in their LIVE form behind label_rows_kernel; the tail is that of the pair joins.
extern "C" int isccsearch_join_within_live(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t n_live, const uint64_t* live_keys,
                                uint64_t capacity, uint64_t* out_keys_a, uint64_t* out_keys_b, uint32_t* out_hamming, uint16_t* out_prefix_bits,
                                uint64_t* out_total) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!max_hamming || !out_total || (n_live && !live_keys)) return fail(-EINVAL, "NULL argument");
    if (capacity && (!out_keys_a || !out_keys_b || !out_hamming || !out_prefix_bits))
        return fail(-EINVAL, "NULL output array with capacity %llu", (unsigned long long)capacity);
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc;
    if ((rc = join_live_check(h, "join_within_live", table, n_live, live_keys, tp))) return rc;
    Table& t = *tp;
    *out_total = 0;
    if (n_live < 2 || table_rows(t) < 2) return 0;     // no pair of listed rows: nothing is launched
    HIPOK(hipSetDevice(h->device));
    JoinPlan plan;
    if ((rc = join_begin(h, plan, isk::JoinForm::LIVE, false, 1, capacity))) return rc;
    uint32_t* row_labels[ISCCSEARCH_MAX_BYTES + 1] = {};
    if ((rc = join_label_rows(h, t, n_live, live_keys, nullptr, row_labels))) return rc;
    rc = join_self_pairs(t, max_hamming, [&](uint32_t a_len, uint32_t b_len, uint32_t pbytes, bool same) {
        return join_add(h, plan, t.seg[a_len], t.seg[b_len], pbytes, max_hamming[pbytes], same, false, row_labels[a_len], row_labels[b_len]);
    });
    if (rc) return rc;
    return join_finish(h, plan, out_keys_a, out_keys_b, out_hamming, out_prefix_bits, out_total);
}

// The overlap joins: isccsearch_join_overlaps and isccsearch_join_segments over ONE side (the self-join of a simprint table's one segment)
// and isccsearch_join_overlaps_between and isccsearch_join_segments_between over TWO (the one cross-join launch isccsearch_join_between
// would make for the two segments, the side with more rows held, by join_add's rule), all in the launches' OVERLAP form.  Per side
// label_chunks_kernel (its own asset keys,
// frequency column, chunks and counters; the host never sees the tables' keys; the second side's labels carry isk::LABEL_SIDE_B), then
// the join launch, then the aggregation of overlap.hip, all on one stream; the counters and the chunks per asset come back behind ONE
// synchronisation, then the records are copied.  The hit buffer is filled with ones first, so that the aggregation runs over
// 2 * capacity slots without the host asking how many were written.  Every frequency column is built before anything of the call is
// queued (each build drains the stream).  Everything the device code relies on -- asset keys ascending and few enough that no label
// is UF_NONE (two sides: 2^31 - 1, the side bit), rows and hit positions below 2^32 -- is checked before anything is launched.
//
// `segments` (isccsearch_join_segments, isccsearch_join_segments_between): the stage of segments.hip is queued between the join launch
// and the aggregation, which overwrites the hit buffer that stage reads.  One side: it is the stage's source and destination.  Two
// sides: table_a is the source and table_b the destination, whichever of them the launch held.  Without the flag nothing of that
// stage is sized, allocated or queued.
//
// Two sides: the sort by (src, dst) puts the records of direction A -> B (src without the side bit) before those of B -> A; the bit moves
// into `reserved` on the host, after the copy.
namespace {
static_assert(isksg::SIDE_B == isk::LABEL_SIDE_B, "segments.hip tells the sides of a cross join apart by the labels' side bit");
struct OverlapSide {
    uint32_t table;               // the caller's arguments
    uint32_t n_assets;
    const uint64_t* asset_keys;
    uint32_t* out_chunks;
    Table* t;                     // the table and its one segment, once the call holds the lock
    Segment* seg;
};
// the call's device counters; out_info is {chunk pairs, records, {live rows, stop chunks} per side, segments if asked for}
enum : uint32_t { OV_PAIRS = 0, OV_RECORDS, OV_SEGMENTS, OV_SIDE /* + 2 * side: live rows, stop chunks */, OV_COUNTERS = OV_SIDE + 4 };

int join_overlap_sides(isccsearch_handle* h, const char* name, OverlapSide* sides, int n_sides, int32_t max_hamming, uint32_t max_doc_freq,
                       uint32_t dup_limit, uint32_t flags, uint64_t capacity, isccsearch_overlap* out_pairs, uint64_t* out_info, bool segments,
                       isccsearch_segment* out_segments) {
    const bool cross = n_sides == 2;
    const char* const suffix[2] = {cross ? "_a" : "", "_b"};
    if (!h) return fail(-EINVAL, "handle is NULL");
    for (int x = 0; x < n_sides; ++x)
        if (!sides[x].asset_keys || !sides[x].out_chunks || !out_info) return fail(-EINVAL, "NULL argument");
    if (capacity && !out_pairs) return fail(-EINVAL, "out_pairs is NULL with capacity %llu", (unsigned long long)capacity);
    if (segments && capacity && !out_segments) return fail(-EINVAL, "out_segments is NULL with capacity %llu", (unsigned long long)capacity);
    if (cross && sides[0].table == sides[1].table)
        return fail(-EINVAL, "%s needs two tables (table %u given twice): isccsearch_join_overlaps joins a table with itself", name, sides[0].table);
    if (flags & ~ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET) return fail(-EINVAL, "unknown flags 0x%x", flags & ~ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET);
    for (int x = 0; x < n_sides; ++x) {
        const uint32_t n = sides[x].n_assets;
        if (cross ? n == 0 || n > 0x7FFFFFFFu : n == 0 || n == isk::UF_NONE)
            return fail(-EINVAL, "n_assets%s must be in 1 .. %s, got %u", suffix[x], cross ? "2^31 - 1" : "2^32 - 2", n);
    }
    for (int x = 0; x < n_sides; ++x)
        if (int rc = check_ascending((std::string("asset_keys") + suffix[x]).c_str(), sides[x].asset_keys, sides[x].n_assets)) return rc;
    if (max_hamming < 0) return fail(-EINVAL, "max_hamming must be >= 0, got %d", max_hamming);
    if (max_doc_freq > 0 && max_doc_freq > dup_limit)
        return fail(-EINVAL, "max_doc_freq %u exceeds dup_limit %u: the frequency column counts no further", max_doc_freq, dup_limit);
    if (capacity >= (1ull << 31))
        return fail(-E2BIG, "capacity %llu: the two hits of a chunk pair are numbered with 32 bits", (unsigned long long)capacity);
    std::lock_guard<std::mutex> lk(h->mu);
    int rc;
    for (int x = 0; x < n_sides; ++x)
        if ((rc = get_table(h, sides[x].table, sides[x].t))) return rc;
    for (int x = 0; x < n_sides; ++x)
        if (sides[x].t->metric != ISCCSEARCH_METRIC_HAMMING || sides[x].t->key_words != 2)
            return fail(-EINVAL, "%s needs %s (HAMMING, key_words 2), table %u has metric %d and key_words %d", name, cross ? "simprint tables" : "a simprint table",
                        sides[x].table, sides[x].t->metric, sides[x].t->key_words);
    if (cross && sides[0].t->max_bytes != sides[1].t->max_bytes)
        return fail(-EINVAL, "simprint tables %u and %u hold codes of different lengths (max_bytes %d, %d)", sides[0].table, sides[1].table,
                    sides[0].t->max_bytes, sides[1].t->max_bytes);
    const uint32_t nbytes = (uint32_t)sides[0].t->max_bytes;
    uint64_t all_assets = 0, all_rows = 0;
    for (int x = 0; x < n_sides; ++x) {
        Segment& s = *(sides[x].seg = &sides[x].t->seg[nbytes]);
        if (s.n >= (1ull << 32))
            return cross ? fail(-E2BIG, "a segment of %llu rows in table %u: row numbers travel as 32 bits", (unsigned long long)s.n, sides[x].table)
                         : fail(-E2BIG, "a segment of %llu rows: row numbers travel as 32 bits", (unsigned long long)s.n);
        if (segments && s.n >= (1ull << 31))
            return cross ? fail(-E2BIG, "a segment of %llu rows in table %u: the difference of two chunk ordinals travels as 32 bits", (unsigned long long)s.n,
                                sides[x].table)
                         : fail(-E2BIG, "a segment of %llu rows: the difference of two chunk ordinals travels as 32 bits", (unsigned long long)s.n);
        all_assets += sides[x].n_assets;
        all_rows += s.n;
    }
    // the side with more rows is held (join_add); one side: it is joined with itself, which takes two rows
    const int held = cross && sides[1].seg->n > sides[0].seg->n ? 1 : 0, streamed = cross ? 1 - held : 0;
    Segment& A = *sides[held].seg;
    Segment& B = *sides[streamed].seg;
    const bool launch = cross ? A.n && B.n : A.n >= 2;
    HIPOK(hipSetDevice(h->device));
    // side by side (A first): asset keys, chunks per asset, row labels; for m = 2 * capacity hits {appended | sorted}, one-hit records,
    // records and rocPRIM's temporary storage: 192 bytes per chunk pair of the capacity.
    // With `segments`, in buffers of their own, for the capacity pair keys {keyed | sorted} and runs {one-pair | reduced}: 160 bytes more per
    // chunk pair; for the rows sorted keys, sorted rows and ordinals: 24 bytes per row, both sides' in one buffer each (the stage's source
    // side first) as the row labels are; rocPRIM's temporary storage is shared, the larger of the two stages' needs.  Nothing is queued
    // for the hits when there is no launch or no room.
    const uint64_t m = 2 * capacity;
    const bool run = m && launch, locate = segments && run;
    // the stage's sides: table_a and table_b, or the one table twice
    const isksg::Side sg_src{reinterpret_cast<const isksg::RowKey*>(sides[0].seg->keys), sides[0].seg->n};
    const isksg::Side sg_dst{reinterpret_cast<const isksg::RowKey*>(sides[n_sides - 1].seg->keys), sides[n_sides - 1].seg->n};
    size_t temp_bytes = 0;
    if ((rc = h->d_join_live_keys.ensure(all_assets))) return rc;
    if ((rc = h->d_ov_chunks.ensure(all_assets))) return rc;
    if ((rc = h->d_join_row_labels.ensure(std::max<uint64_t>(all_rows, 1)))) return rc;
    if (m) {
        std::string err;
        if ((rc = iskov::aggregate_temp_bytes(m, &temp_bytes, &err))) return fail(rc, "%s", err.c_str());
        if (locate) {
            size_t locate_bytes = 0;
            if ((rc = isksg::locate_temp_bytes(sg_src.n, sg_dst.n, capacity, &locate_bytes, &err))) return fail(rc, "%s", err.c_str());
            temp_bytes = std::max(temp_bytes, locate_bytes);
            if ((rc = h->d_sg_keys.ensure(all_rows))) return rc;
            if ((rc = h->d_sg_rows.ensure(2 * all_rows))) return rc;
            if ((rc = h->d_sg_pairs.ensure(m))) return rc;
            if ((rc = h->d_sg_runs.ensure(m))) return rc;
        }
        if ((rc = h->d_ov_hits.ensure(2 * m))) return rc;
        if ((rc = h->d_ov_marks.ensure(m))) return rc;
        if ((rc = h->d_ov_records.ensure(m))) return rc;
        if ((rc = h->d_ov_temp.ensure(std::max<size_t>(temp_bytes, 1)))) return rc;
    }
    // (a frequency column is built by a call of its own that drains the stream: nothing of this call is queued yet)
    for (int x = 0; x < n_sides; ++x)
        if (max_doc_freq > 0 && sides[x].seg->n && (rc = ensure_freq_column(h, *sides[x].t, *sides[x].seg, dup_limit))) return rc;
    JoinPlan plan;
    if ((rc = join_begin(h, plan, isk::JoinForm::OVERLAP, cross, 2, capacity, OV_COUNTERS))) return rc;
    unsigned long long* const counters = reinterpret_cast<unsigned long long*>(h->d_join_total.p);
    HIPOK(hipMemsetAsync(h->d_ov_chunks.p, 0, (size_t)all_assets * 4, h->stream));
    if (run) HIPOK(hipMemsetAsync(h->d_ov_hits.p, 0xFF, m * sizeof(iskov::Hit), h->stream));
    uint32_t* row_labels[2] = {h->d_join_row_labels.p, h->d_join_row_labels.p + sides[0].seg->n};
    const uint64_t first_asset[2] = {0, sides[0].n_assets};
    for (int x = 0; x < n_sides; ++x) {
        uint64_t* const d_keys = h->d_join_live_keys.p + first_asset[x];
        HIPOK(hipMemcpyAsync(d_keys, sides[x].asset_keys, (size_t)sides[x].n_assets * 8, hipMemcpyHostToDevice, h->stream));
        const Segment& s = *sides[x].seg;
        if (!s.n) continue;
        isk::OverlapLabelParams lp{s.keys, d_keys, max_doc_freq > 0 ? s.freq : nullptr, row_labels[x], h->d_ov_chunks.p + first_asset[x],
                                   counters + OV_SIDE + 2 * x, counters + OV_SIDE + 2 * x + 1, s.n, sides[x].n_assets, max_doc_freq,
                                   x ? isk::LABEL_SIDE_B : 0u};
        hipLaunchKernelGGL(isk::label_chunks_kernel, dim3(row_blocks(s.n)), dim3(isk::BLOCK), 0, h->stream, lp);
        HIPOK(hipGetLastError());
    }
    if (launch) {
        plan.out_hits = reinterpret_cast<uint4*>(h->d_ov_hits.p);
        plan.skip_same_key = (flags & ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET) != 0;
        if ((rc = join_add(h, plan, A, B, nbytes, max_hamming, !cross, held == 1, row_labels[held], row_labels[streamed]))) return rc;
        if ((rc = join_run(h, plan))) return rc;
    }
    if (locate) {                                     // reads the hits the aggregation below overwrites
        std::string err;
        if ((rc = isksg::locate(sg_src, sg_dst, h->d_ov_hits.p, capacity, h->d_sg_keys.p, h->d_sg_rows.p, h->d_sg_rows.p + all_rows, h->d_sg_pairs.p,
                                h->d_sg_runs.p, counters + OV_SEGMENTS, h->d_ov_temp.p, temp_bytes, h->stream, &err)))
            return fail(rc, "%s", err.c_str());
    }
    if (run) {
        std::string err;
        if ((rc = iskov::aggregate(h->d_ov_hits.p, h->d_ov_hits.p + m, h->d_ov_marks.p, h->d_ov_records.p, counters + OV_RECORDS, m, h->d_ov_temp.p,
                                   temp_bytes, h->stream, &err)))
            return fail(rc, "%s", err.c_str());
    }
    // the call's one synchronisation; the outputs change only from here on
    uint64_t got[OV_COUNTERS] = {};
    std::vector<uint32_t> chunks(all_assets);
    HIPOK(hipMemcpyAsync(got, counters, sizeof got, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(chunks.data(), h->d_ov_chunks.p, (size_t)all_assets * 4, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    const uint64_t total = got[OV_PAIRS];
    if (total > capacity) {
        out_info[0] = total;
        return fail(-ENOSPC, "%llu chunk pairs do not fit the capacity of %llu", (unsigned long long)total, (unsigned long long)capacity);
    }
    // (slots were left unused: the run of ones behind the hits reduced to one more record, the last; likewise the one run of the unused slots)
    const uint64_t unused = total < capacity ? 1 : 0;
    const uint64_t n_records = run ? got[OV_RECORDS] - unused : 0;
    const uint64_t n_segments = locate ? got[OV_SEGMENTS] - unused : 0;
    if (n_records) HIPOK(hipMemcpyAsync(out_pairs, h->d_ov_records.p, n_records * sizeof(isccsearch_overlap), hipMemcpyDeviceToHost, h->stream));
    if (n_segments)
        HIPOK(hipMemcpyAsync(out_segments, h->d_sg_runs.p + capacity, n_segments * sizeof(isccsearch_segment), hipMemcpyDeviceToHost, h->stream));
    if (n_records || n_segments) HIPOK(hipStreamSynchronize(h->stream));
    // the side bit of src becomes the direction; the order by (src, dst) with the bit is the order by (reserved, src, dst) without
    for (uint64_t r = 0; cross && r < n_records; ++r) {
        isccsearch_overlap& o = out_pairs[r];
        o.reserved = o.src >> 31;
        o.src &= ~isk::LABEL_SIDE_B;
        o.dst &= ~isk::LABEL_SIDE_B;
    }
    uint64_t* info = out_info;
    *info++ = total;
    *info++ = n_records;
    for (int x = 0; x < n_sides; ++x) {
        memcpy(sides[x].out_chunks, chunks.data() + first_asset[x], (size_t)sides[x].n_assets * 4);
        *info++ = got[OV_SIDE + 2 * x];
        *info++ = got[OV_SIDE + 2 * x + 1];
    }
    if (segments) *info++ = n_segments;
    return 0;
}
}  // namespace

extern "C" int isccsearch_join_overlaps(isccsearch_handle* h, uint32_t table, int32_t max_hamming, uint32_t max_doc_freq, uint32_t dup_limit,
                             uint32_t n_assets, const uint64_t* asset_keys, uint64_t capacity, isccsearch_overlap* out_pairs,
                             uint32_t* out_chunks, uint64_t* out_info) {
    OverlapSide side{table, n_assets, asset_keys, out_chunks, nullptr, nullptr};
    return join_overlap_sides(h, "join_overlaps", &side, 1, max_hamming, max_doc_freq, dup_limit, 0, capacity, out_pairs, out_info, false, nullptr);
}

// isccsearch_join_overlaps and, from the same join launch, the chunk pairs of every pair of assets as aligned runs (segments.hip).
extern "C" int isccsearch_join_segments(isccsearch_handle* h, uint32_t table, int32_t max_hamming, uint32_t max_doc_freq, uint32_t dup_limit,
                             uint32_t n_assets, const uint64_t* asset_keys, uint64_t capacity, isccsearch_overlap* out_pairs,
                             isccsearch_segment* out_segments, uint32_t* out_chunks, uint64_t* out_info) {
    OverlapSide side{table, n_assets, asset_keys, out_chunks, nullptr, nullptr};
    return join_overlap_sides(h, "join_segments", &side, 1, max_hamming, max_doc_freq, dup_limit, 0, capacity, out_pairs, out_info, true, out_segments);
}

// isccsearch_join_overlaps between TWO simprint tables.
extern "C" int isccsearch_join_overlaps_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b, int32_t max_hamming,
                                     uint32_t max_doc_freq, uint32_t dup_limit, uint32_t n_assets_a, const uint64_t* asset_keys_a,
                                     uint32_t n_assets_b, const uint64_t* asset_keys_b, uint32_t flags, uint64_t capacity,
                                     isccsearch_overlap* out_pairs, uint32_t* out_chunks_a, uint32_t* out_chunks_b, uint64_t* out_info) {
    OverlapSide sides[2] = {{table_a, n_assets_a, asset_keys_a, out_chunks_a, nullptr, nullptr}, {table_b, n_assets_b, asset_keys_b, out_chunks_b, nullptr, nullptr}};
    return join_overlap_sides(h, "join_overlaps_between", sides, 2, max_hamming, max_doc_freq, dup_limit, flags, capacity, out_pairs, out_info, false, nullptr);
}

// isccsearch_join_overlaps_between and, from the same join launch, the chunk pairs of every pair (asset of table_a, asset of table_b) as
// aligned runs (segments.hip, table_a its source side and table_b its destination side).
extern "C" int isccsearch_join_segments_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b, int32_t max_hamming,
                                     uint32_t max_doc_freq, uint32_t dup_limit, uint32_t n_assets_a, const uint64_t* asset_keys_a,
                                     uint32_t n_assets_b, const uint64_t* asset_keys_b, uint32_t flags, uint64_t capacity,
                                     isccsearch_overlap* out_pairs, isccsearch_segment* out_segments, uint32_t* out_chunks_a, uint32_t* out_chunks_b,
                                     uint64_t* out_info) {
    OverlapSide sides[2] = {{table_a, n_assets_a, asset_keys_a, out_chunks_a, nullptr, nullptr}, {table_b, n_assets_b, asset_keys_b, out_chunks_b, nullptr, nullptr}};
    return join_overlap_sides(h, "join_segments_between", sides, 2, max_hamming, max_doc_freq, dup_limit, flags, capacity, out_pairs, out_info, true, out_segments);
}
