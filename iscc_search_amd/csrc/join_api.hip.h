// join_api.hip.h -- isccsearch_join_within and isccsearch_join_between: the self-join of a table and the cross join of two
// tables by the XOR + popcount kernel of join.hip.h or, for launches over enough rows, its matrix-core form (mfma_join_kernel.hip.h);
// and isccsearch_join_components: the self-join's launches in their LINK form, whose pairs are united in a union-find array
// (unionfind.hip.h) instead of written; and isccsearch_join_overlaps: the self-join of a simprint table in the launches' OVERLAP form,
// whose directed hits overlap.hip sorts and reduces to one record per ordered pair of assets; and isccsearch_join_segments: the same
// call, whose chunk pairs segments.hip turns into aligned runs before they are reduced; and isccsearch_join_overlaps_between: the
// cross join of two simprint tables in the same OVERLAP form, with a label space per table.
// Needs the store of isccsearch.hip (Segment, Table; get_table of store.hip.h) and its scratch buffers.
namespace {
// one launch of the join kernel (join.hip.h)
template <int W, bool CROSS, bool LINK, bool OVERLAP>
void launch_join(const isk::JoinParams& jp, bool mask, uint64_t blocks, hipStream_t stream) {
    if (mask) hipLaunchKernelGGL((isk::join_scan_kernel<W, true, CROSS, LINK, OVERLAP>), dim3((uint32_t)blocks), dim3(isk::BLOCK), 0, stream, jp);
    else hipLaunchKernelGGL((isk::join_scan_kernel<W, false, CROSS, LINK, OVERLAP>), dim3((uint32_t)blocks), dim3(isk::BLOCK), 0, stream, jp);
}
template <bool CROSS, bool LINK = false, bool OVERLAP = false>
void launch_join(uint32_t W, const isk::JoinParams& jp, bool mask, uint64_t blocks, hipStream_t stream) {
    switch (W) {
        case 1: launch_join<1, CROSS, LINK, OVERLAP>(jp, mask, blocks, stream); break;
        case 2: launch_join<2, CROSS, LINK, OVERLAP>(jp, mask, blocks, stream); break;
        case 3: launch_join<3, CROSS, LINK, OVERLAP>(jp, mask, blocks, stream); break;
        default: launch_join<4, CROSS, LINK, OVERLAP>(jp, mask, blocks, stream); break;
    }
}
constexpr uint32_t join_rows_per_block(uint32_t W) {
    return W == 1 ? isk::join_rows_per_block<1>() : W == 2 ? isk::join_rows_per_block<2>() : W == 3 ? isk::join_rows_per_block<3>() : isk::join_rows_per_block<4>();
}

// One call's launches: one per pair of segments, all appending to one output.  What only the emit path reads goes to the
// device as one array of descriptors.
struct JoinPlan {
    // mfma: the launch takes mfma_join_kernel (mp, chunks of `groups` * 32 held rows), else join_scan_kernel (jp, blocks)
    struct Launch { isk::JoinParams jp; uint32_t W; bool mask; uint64_t blocks; bool mfma; isk::MfmaJoinParams mp; uint32_t groups; uint64_t chunks; };
    std::vector<Launch> launches;
    std::vector<isk::JoinEmit> emits;
    bool cross = false;
    bool link = false;     // isccsearch_join_components: the LINK form of either kernel (JoinEmit::labels_a, labels_b, parent are set)
    bool overlap = false;  // isccsearch_join_overlaps: the OVERLAP form of either kernel (JoinEmit::labels_a, labels_b, out_hits are set);
                           // with `cross`: isccsearch_join_overlaps_between
    uint32_t KW = 1;
    uint64_t capacity = 0, cap_alloc = 1;
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

// the output buffers of one call and its pair counter, zeroed
int join_begin(isccsearch_handle* h, JoinPlan& plan, bool cross, uint32_t KW, uint64_t capacity) {
    plan.cross = cross;
    plan.KW = KW;
    plan.capacity = capacity;
    plan.cap_alloc = std::max<uint64_t>(capacity, 1);
    int rc;
    if ((rc = h->d_join_keys.ensure(plan.cap_alloc * 2 * KW))) return rc;
    if ((rc = h->d_join_ham.ensure(plan.cap_alloc))) return rc;
    if ((rc = h->d_join_pb.ensure(plan.cap_alloc))) return rc;
    if ((rc = h->d_join_total.ensure(1))) return rc;
    HIPOK(hipMemsetAsync(h->d_join_total.p, 0, 8, h->stream));
    return 0;
}

// One launch: segment A (one block per TQ rows, the rows in SGPRs) against segment B (streamed by every block) over a common
// prefix of pbytes bytes under tau.  `same`: A and B are one segment (the self-join keeps row_a < row_b).  `sgpr_side_is_b`:
// a cross join whose segment A belongs to the call's table_b.
// On the matrix cores (options mfma, join_mfma; both segments of at least join_mfma_min_rows rows) segment A is the HELD side --
// chunks of its rows in LDS, what the SGPRs are to join_scan_kernel -- and B is streamed: the same roles, the same JoinEmit.
int join_add(isccsearch_handle* h, JoinPlan& plan, Segment& A, Segment& B, uint32_t pbytes, int tau, bool same, bool sgpr_side_is_b) {
    const uint32_t W = (pbytes + 7) / 8;
    JoinPlan::Launch L{};
    set_cols(L.jp.col_a, A, W);
    set_cols(L.jp.col_b, B, W);
    L.jp.n_a = A.n; L.jp.n_b = B.n;
    L.jp.mask = mask_for(pbytes);
    L.jp.tau = (uint32_t)std::min<int>(tau, 8 * ISCCSEARCH_MAX_BYTES);
    L.jp.same = same ? 1u : 0u;
    isk::JoinEmit e{};
    e.keys_a = A.keys; e.keys_b = B.keys;
    e.n_a = A.n;
    e.capacity = plan.capacity;
    e.total = reinterpret_cast<unsigned long long*>(h->d_join_total.p);
    e.out_keys_a = h->d_join_keys.p;
    e.out_keys_b = h->d_join_keys.p + plan.cap_alloc * plan.KW;
    e.out_hamming = h->d_join_ham.p;
    e.out_prefix_bits = h->d_join_pb.p;
    e.prefix_bits = 8 * pbytes;
    e.kw = plan.KW;
    e.sgpr_side_is_b = sgpr_side_is_b ? 1u : 0u;
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
        // (any count from 2^20 rows on sizes the chunk alike: as many groups as 40 KB of LDS hold)
        L.groups = isk::mfma_groups_per_chunk((int)W, (uint32_t)std::min<uint64_t>(A.n, 1u << 20), false);
        L.chunks = (A.n + L.groups * 32 - 1) / (L.groups * 32);
    }
    plan.launches.push_back(L);
    plan.emits.push_back(e);
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
                    const int lrc = isk::launch_mfma_join((int)L.W, plan.cross, blocks_x, chunks, L.groups, h->stream, L.mp, plan.link, plan.overlap);
                    if (lrc) return fail(-EINVAL, "the matrix-core join does not take chunks of %u groups of %u words", L.groups, L.W);
                    HIPOK(hipGetLastError());
                    h->stats.join_launches += 1;
                    h->stats.join_mfma_launches += 1;
                }
                continue;
            }
            if (plan.overlap && plan.cross) launch_join<true, false, true>(L.W, L.jp, L.mask, L.blocks, h->stream);
            else if (plan.overlap) launch_join<false, false, true>(L.W, L.jp, L.mask, L.blocks, h->stream);
            else if (plan.link) launch_join<false, true>(L.W, L.jp, L.mask, L.blocks, h->stream);
            else if (plan.cross) launch_join<true>(L.W, L.jp, L.mask, L.blocks, h->stream);
            else launch_join<false>(L.W, L.jp, L.mask, L.blocks, h->stream);
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
    if ((rc = join_begin(h, plan, false, (uint32_t)t.key_words, capacity))) return rc;
    // one launch per pair of segments (la <= lb: the pair compares la bytes under max_hamming[la])
    for (uint32_t la = 1; la <= ISCCSEARCH_MAX_BYTES; ++la) {
        if (!t.seg[la].n || max_hamming[la] < 0) continue;
        for (uint32_t lb = la; lb <= ISCCSEARCH_MAX_BYTES; ++lb) {
            const bool same = la == lb;
            if (!t.seg[lb].n || (same && t.seg[la].n < 2)) continue;
            // side A (one block per TQ rows, or held in LDS chunk by chunk) is the segment with more rows; side B is streamed by every block
            Segment& A = t.seg[lb].n > t.seg[la].n ? t.seg[lb] : t.seg[la];
            Segment& B = &A == &t.seg[la] ? t.seg[lb] : t.seg[la];
            if ((rc = join_add(h, plan, A, B, la, max_hamming[la], same, false))) return rc;
        }
    }
    return join_finish(h, plan, out_keys_a, out_keys_b, out_hamming, out_prefix_bits, out_total);
}

// One cross-join launch (join_scan_kernel<W, MASK, true> or mfma_join_kernel<W, true>) per pair of non-empty segments (la of table_a, lb of table_b), in either order of
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
    if ((rc = join_begin(h, plan, true, (uint32_t)ta->key_words, capacity))) return rc;
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

// The launches of isccsearch_join_within in their LINK form (join_scan_kernel<W, MASK, false, true> / mfma_join_kernel<W, false, true>)
// between label_rows_kernel (one per segment: the host never sees the table's keys) and flatten_kernel, all on one stream; then
// `parent` and the links come back behind one synchronisation.  Everything the device code relies on -- labels < n_labels,
// parent[i] <= i -- is checked on the host before anything is launched.
extern "C" int isccsearch_join_components(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t n_live,
                               const uint64_t* live_keys, const uint32_t* live_labels, uint32_t n_labels, uint32_t* parent,
                               uint64_t* out_links) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!max_hamming || !parent || !out_links || (n_live && (!live_keys || !live_labels))) return fail(-EINVAL, "NULL argument");
    *out_links = 0;
    if (n_labels == 0 || n_labels == isk::UF_NONE) return fail(-EINVAL, "n_labels must be in 1 .. 2^32 - 2, got %u", n_labels);
    for (uint64_t i = 0; i < n_live; ++i) {
        if (i && live_keys[i] <= live_keys[i - 1])
            return fail(-EINVAL, "live_keys must be strictly ascending: live_keys[%llu] <= live_keys[%llu]", (unsigned long long)i, (unsigned long long)(i - 1));
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
    plan.link = true;
    if ((rc = join_begin(h, plan, false, 1, 0))) return rc;
    if ((rc = h->d_join_live_keys.ensure(std::max<uint64_t>(n_live, 1)))) return rc;
    if ((rc = h->d_join_live_labels.ensure(std::max<uint64_t>(n_live, 1)))) return rc;
    uint64_t all_rows = 0;
    for (uint32_t l = 1; l <= ISCCSEARCH_MAX_BYTES; ++l) all_rows += t.seg[l].n;
    if ((rc = h->d_join_row_labels.ensure(std::max<uint64_t>(all_rows, 1)))) return rc;
    if ((rc = h->d_join_parent.ensure(n_labels))) return rc;
    if (n_live) {
        HIPOK(hipMemcpyAsync(h->d_join_live_keys.p, live_keys, n_live * 8, hipMemcpyHostToDevice, h->stream));
        HIPOK(hipMemcpyAsync(h->d_join_live_labels.p, live_labels, n_live * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIPOK(hipMemcpyAsync(h->d_join_parent.p, parent, (size_t)n_labels * 4, hipMemcpyHostToDevice, h->stream));
    // a label per row, segment by segment
    uint32_t* row_labels[ISCCSEARCH_MAX_BYTES + 1] = {};
    uint64_t rows = 0;
    for (uint32_t l = 1; l <= ISCCSEARCH_MAX_BYTES; ++l) {
        const Segment& s = t.seg[l];
        if (!s.n) continue;
        row_labels[l] = h->d_join_row_labels.p + rows;
        rows += s.n;
        isk::LabelParams lp{s.keys, h->d_join_live_keys.p, h->d_join_live_labels.p, row_labels[l], s.n, n_live};
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((s.n + isk::BLOCK - 1) / isk::BLOCK, 1u << 16);
        hipLaunchKernelGGL(isk::label_rows_kernel, dim3(blocks), dim3(isk::BLOCK), 0, h->stream, lp);
        HIPOK(hipGetLastError());
    }
    // the launches of isccsearch_join_within
    for (uint32_t la = 1; la <= ISCCSEARCH_MAX_BYTES; ++la) {
        if (!t.seg[la].n || max_hamming[la] < 0) continue;
        for (uint32_t lb = la; lb <= ISCCSEARCH_MAX_BYTES; ++lb) {
            const bool same = la == lb;
            if (!t.seg[lb].n || (same && t.seg[la].n < 2)) continue;
            const uint32_t a_len = t.seg[lb].n > t.seg[la].n ? lb : la, b_len = a_len == la ? lb : la;
            if ((rc = join_add(h, plan, t.seg[a_len], t.seg[b_len], la, max_hamming[la], same, false))) return rc;
            isk::JoinEmit& e = plan.emits.back();
            e.labels_a = row_labels[a_len];
            e.labels_b = row_labels[b_len];
            e.parent = h->d_join_parent.p;
        }
    }
    if ((rc = join_run(h, plan))) return rc;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_labels + isk::BLOCK - 1) / isk::BLOCK, 1u << 16);
    hipLaunchKernelGGL(isk::flatten_kernel, dim3(blocks), dim3(isk::BLOCK), 0, h->stream, h->d_join_parent.p, n_labels);
    HIPOK(hipGetLastError());
    // the array goes to a copy first: `parent` changes only once the whole call has succeeded
    std::vector<uint32_t> flat(n_labels);
    HIPOK(hipMemcpyAsync(flat.data(), h->d_join_parent.p, (size_t)n_labels * 4, hipMemcpyDeviceToHost, h->stream));
    if ((rc = join_total(h, out_links))) return rc;
    memcpy(parent, flat.data(), (size_t)n_labels * 4);
    return 0;
}

// The self-join launch of a simprint table's one segment in its OVERLAP form (join_scan_kernel<W, MASK, false, false, true> /
// mfma_join_kernel<W, false, false, true>, chosen by join_add's rule) between label_chunks_kernel (the host never sees the table's keys)
// and the aggregation of overlap.hip, all on one stream; the counters and the chunks per asset come back behind ONE synchronisation,
// then the records are copied.  The hit buffer is filled with ones first, so that the aggregation runs over 2 * capacity slots
// without the host asking how many were written.  Everything the device code relies on -- asset_keys ascending and fewer than
// 2^32 - 1 (labels and the bound of the label search), rows and hit positions below 2^32 -- is checked before anything is launched.
//
// `segments` (isccsearch_join_segments): the same call with the stage of segments.hip queued between the join launch and the
// aggregation, which overwrites the hit buffer that stage reads; the segment count is the call's fifth counter and comes back behind
// the same synchronisation.  Without the flag nothing of that stage is sized, allocated or queued.
namespace {
int join_overlaps_or_segments(isccsearch_handle* h, uint32_t table, int32_t max_hamming, uint32_t max_doc_freq, uint32_t dup_limit,
                              uint32_t n_assets, const uint64_t* asset_keys, uint64_t capacity, isccsearch_overlap* out_pairs,
                              uint32_t* out_chunks, uint64_t* out_info, bool segments, isccsearch_segment* out_segments) {
    const char* const name = segments ? "join_segments" : "join_overlaps";
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!asset_keys || !out_chunks || !out_info) return fail(-EINVAL, "NULL argument");
    if (capacity && !out_pairs) return fail(-EINVAL, "out_pairs is NULL with capacity %llu", (unsigned long long)capacity);
    if (segments && capacity && !out_segments) return fail(-EINVAL, "out_segments is NULL with capacity %llu", (unsigned long long)capacity);
    if (n_assets == 0 || n_assets == isk::UF_NONE) return fail(-EINVAL, "n_assets must be in 1 .. 2^32 - 2, got %u", n_assets);
    for (uint32_t i = 1; i < n_assets; ++i)
        if (asset_keys[i] <= asset_keys[i - 1])
            return fail(-EINVAL, "asset_keys must be strictly ascending: asset_keys[%u] <= asset_keys[%u]", i, i - 1);
    if (max_hamming < 0) return fail(-EINVAL, "max_hamming must be >= 0, got %d", max_hamming);
    if (max_doc_freq > 0 && max_doc_freq > dup_limit)
        return fail(-EINVAL, "max_doc_freq %u exceeds dup_limit %u: the frequency column counts no further", max_doc_freq, dup_limit);
    if (capacity >= (1ull << 31))
        return fail(-E2BIG, "capacity %llu: the two hits of a chunk pair are numbered with 32 bits", (unsigned long long)capacity);
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc;
    if ((rc = get_table(h, table, tp))) return rc;
    Table& t = *tp;
    if (t.metric != ISCCSEARCH_METRIC_HAMMING || t.key_words != 2)
        return fail(-EINVAL, "%s needs a simprint table (HAMMING, key_words 2), table %u has metric %d and key_words %d", name, table, t.metric, t.key_words);
    Segment& s = t.seg[t.max_bytes];
    if (s.n >= (1ull << 32)) return fail(-E2BIG, "a segment of %llu rows: row numbers travel as 32 bits", (unsigned long long)s.n);
    if (segments && s.n >= (1ull << 31))
        return fail(-E2BIG, "a segment of %llu rows: the difference of two chunk ordinals travels as 32 bits", (unsigned long long)s.n);
    HIPOK(hipSetDevice(h->device));
    // the call's counters {chunk pairs, live rows, stop chunks, records}, asset keys, chunks per asset, row labels; for m = 2 * capacity
    // hits {appended | sorted}, one-hit records, records and rocPRIM's temporary storage: 192 bytes per chunk pair of the capacity
    // With `segments` a fifth counter {segments} and, in buffers of their own, for the capacity pair keys {keyed | sorted} and runs
    // {one-pair | reduced}: 160 bytes more per chunk pair; for the rows sorted keys, sorted rows and ordinals: 24 bytes per row;
    // rocPRIM's temporary storage is shared, the larger of the two stages' needs.  The stage runs when there is a pair of rows and room.
    const uint64_t m = 2 * capacity;
    const uint32_t n_counters = segments ? 5 : 4;
    const bool locate = segments && capacity && s.n >= 2;
    size_t temp_bytes = 0;
    if ((rc = h->d_join_total.ensure(n_counters))) return rc;
    if ((rc = h->d_join_live_keys.ensure(n_assets))) return rc;
    if ((rc = h->d_ov_chunks.ensure(n_assets))) return rc;
    if ((rc = h->d_join_row_labels.ensure(std::max<uint64_t>(s.n, 1)))) return rc;
    if (m) {
        std::string err;
        if ((rc = iskov::aggregate_temp_bytes(m, &temp_bytes, &err))) return fail(rc, "%s", err.c_str());
        if (locate) {
            size_t locate_bytes = 0;
            if ((rc = isksg::locate_temp_bytes(s.n, capacity, &locate_bytes, &err))) return fail(rc, "%s", err.c_str());
            temp_bytes = std::max(temp_bytes, locate_bytes);
            if ((rc = h->d_sg_keys.ensure(s.n))) return rc;
            if ((rc = h->d_sg_rows.ensure(2 * s.n))) return rc;
            if ((rc = h->d_sg_pairs.ensure(m))) return rc;
            if ((rc = h->d_sg_runs.ensure(m))) return rc;
        }
        if ((rc = h->d_ov_hits.ensure(2 * m))) return rc;
        if ((rc = h->d_ov_marks.ensure(m))) return rc;
        if ((rc = h->d_ov_records.ensure(m))) return rc;
        if ((rc = h->d_ov_temp.ensure(std::max<size_t>(temp_bytes, 1)))) return rc;
    }
    // (the frequency column is built by a call of its own that drains the stream: nothing of this call is queued yet)
    if (max_doc_freq > 0 && s.n && (rc = ensure_freq_column(h, t, s, dup_limit))) return rc;
    unsigned long long* const counters = reinterpret_cast<unsigned long long*>(h->d_join_total.p);
    HIPOK(hipMemsetAsync(counters, 0, n_counters * 8, h->stream));
    HIPOK(hipMemsetAsync(h->d_ov_chunks.p, 0, (size_t)n_assets * 4, h->stream));
    if (m) HIPOK(hipMemsetAsync(h->d_ov_hits.p, 0xFF, m * sizeof(iskov::Hit), h->stream));
    HIPOK(hipMemcpyAsync(h->d_join_live_keys.p, asset_keys, (size_t)n_assets * 8, hipMemcpyHostToDevice, h->stream));
    if (s.n) {
        isk::OverlapLabelParams lp{s.keys, h->d_join_live_keys.p, max_doc_freq > 0 ? s.freq : nullptr, h->d_join_row_labels.p, h->d_ov_chunks.p,
                                   counters, s.n, n_assets, max_doc_freq, 0u};
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((s.n + isk::BLOCK - 1) / isk::BLOCK, 1u << 16);
        hipLaunchKernelGGL(isk::label_chunks_kernel, dim3(blocks), dim3(isk::BLOCK), 0, h->stream, lp);
        HIPOK(hipGetLastError());
    }
    if (s.n >= 2) {
        JoinPlan plan;
        plan.overlap = true;
        plan.KW = 2;
        plan.capacity = capacity;
        if ((rc = join_add(h, plan, s, s, (uint32_t)t.max_bytes, max_hamming, true, false))) return rc;
        isk::JoinEmit& e = plan.emits.back();
        e.out_keys_a = e.out_keys_b = nullptr;        // the pair form's outputs: not this form's
        e.out_hamming = nullptr;
        e.out_prefix_bits = nullptr;
        e.labels_a = e.labels_b = h->d_join_row_labels.p;
        e.out_hits = reinterpret_cast<uint4*>(h->d_ov_hits.p);
        if ((rc = join_run(h, plan))) return rc;
    }
    if (locate) {                                     // reads the hits the aggregation below overwrites
        std::string err;
        if ((rc = isksg::locate(reinterpret_cast<const isksg::RowKey*>(s.keys), s.n, h->d_ov_hits.p, capacity, h->d_sg_keys.p, h->d_sg_rows.p,
                                h->d_sg_rows.p + s.n, h->d_sg_pairs.p, h->d_sg_runs.p, counters + 4, h->d_ov_temp.p, temp_bytes, h->stream, &err)))
            return fail(rc, "%s", err.c_str());
    }
    if (m) {
        std::string err;
        if ((rc = iskov::aggregate(h->d_ov_hits.p, h->d_ov_hits.p + m, h->d_ov_marks.p, h->d_ov_records.p, counters + 3, m, h->d_ov_temp.p,
                                   temp_bytes, h->stream, &err)))
            return fail(rc, "%s", err.c_str());
    }
    // the call's one synchronisation; the outputs change only from here on
    uint64_t got[5] = {0, 0, 0, 0, 0};
    std::vector<uint32_t> chunks(n_assets);
    HIPOK(hipMemcpyAsync(got, counters, n_counters * 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(chunks.data(), h->d_ov_chunks.p, (size_t)n_assets * 4, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    const uint64_t total = got[0];
    if (total > capacity) {
        out_info[0] = total;
        return fail(-ENOSPC, "%llu chunk pairs do not fit the capacity of %llu", (unsigned long long)total, (unsigned long long)capacity);
    }
    // (slots were left unused: the run of ones behind the hits reduced to one more record, the last)
    const uint64_t n_records = m ? got[3] - (total < capacity ? 1 : 0) : 0;
    const uint64_t n_segments = locate ? got[4] - (total < capacity ? 1 : 0) : 0;       // (likewise the one run of the unused slots)
    if (n_records) HIPOK(hipMemcpyAsync(out_pairs, h->d_ov_records.p, n_records * sizeof(isccsearch_overlap), hipMemcpyDeviceToHost, h->stream));
    if (n_segments)
        HIPOK(hipMemcpyAsync(out_segments, h->d_sg_runs.p + capacity, n_segments * sizeof(isccsearch_segment), hipMemcpyDeviceToHost, h->stream));
    if (n_records || n_segments) HIPOK(hipStreamSynchronize(h->stream));
    memcpy(out_chunks, chunks.data(), (size_t)n_assets * 4);
    out_info[0] = total; out_info[1] = n_records; out_info[2] = got[1]; out_info[3] = got[2];
    if (segments) out_info[4] = n_segments;
    return 0;
}
}  // namespace

extern "C" int isccsearch_join_overlaps(isccsearch_handle* h, uint32_t table, int32_t max_hamming, uint32_t max_doc_freq, uint32_t dup_limit,
                             uint32_t n_assets, const uint64_t* asset_keys, uint64_t capacity, isccsearch_overlap* out_pairs,
                             uint32_t* out_chunks, uint64_t* out_info) {
    return join_overlaps_or_segments(h, table, max_hamming, max_doc_freq, dup_limit, n_assets, asset_keys, capacity, out_pairs, out_chunks, out_info,
                                     false, nullptr);
}

// isccsearch_join_overlaps and, from the same join launch, the chunk pairs of every pair of assets as aligned runs (segments.hip).
extern "C" int isccsearch_join_segments(isccsearch_handle* h, uint32_t table, int32_t max_hamming, uint32_t max_doc_freq, uint32_t dup_limit,
                             uint32_t n_assets, const uint64_t* asset_keys, uint64_t capacity, isccsearch_overlap* out_pairs,
                             isccsearch_segment* out_segments, uint32_t* out_chunks, uint64_t* out_info) {
    return join_overlaps_or_segments(h, table, max_hamming, max_doc_freq, dup_limit, n_assets, asset_keys, capacity, out_pairs, out_chunks, out_info,
                                     true, out_segments);
}

// isccsearch_join_overlaps between TWO simprint tables: label_chunks_kernel once per table (its own asset keys, frequency column,
// chunks and counters; table B's labels carry isk::LABEL_SIDE_B), then the ONE cross-join launch isccsearch_join_between would make for
// the two segments in its OVERLAP form (join_scan_kernel<W, MASK, true, false, true> / mfma_join_kernel<W, true, false, true>, the
// table with more rows held, by join_add's rule), then the aggregation of overlap.hip, all on one stream.  The sort by (src, dst)
// puts the records of direction A -> B (src without the bit) before those of B -> A; the bit moves into `reserved` on the host, after
// the copy.  Both frequency columns are built before anything of the call is queued (each build drains the stream).  Everything the
// device code relies on -- both key arrays ascending and shorter than 2^31 - 1 (labels with the side bit stay below UF_NONE), rows and
// hit positions below 2^32 -- is checked before anything is launched.
extern "C" int isccsearch_join_overlaps_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b, int32_t max_hamming,
                                     uint32_t max_doc_freq, uint32_t dup_limit, uint32_t n_assets_a, const uint64_t* asset_keys_a,
                                     uint32_t n_assets_b, const uint64_t* asset_keys_b, uint32_t flags, uint64_t capacity,
                                     isccsearch_overlap* out_pairs, uint32_t* out_chunks_a, uint32_t* out_chunks_b, uint64_t* out_info) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!asset_keys_a || !asset_keys_b || !out_chunks_a || !out_chunks_b || !out_info) return fail(-EINVAL, "NULL argument");
    if (capacity && !out_pairs) return fail(-EINVAL, "out_pairs is NULL with capacity %llu", (unsigned long long)capacity);
    if (table_a == table_b)
        return fail(-EINVAL, "join_overlaps_between needs two tables (table %u given twice): isccsearch_join_overlaps joins a table with itself", table_a);
    if (flags & ~ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET) return fail(-EINVAL, "unknown flags 0x%x", flags & ~ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET);
    if (n_assets_a == 0 || n_assets_a > 0x7FFFFFFFu) return fail(-EINVAL, "n_assets_a must be in 1 .. 2^31 - 1, got %u", n_assets_a);
    if (n_assets_b == 0 || n_assets_b > 0x7FFFFFFFu) return fail(-EINVAL, "n_assets_b must be in 1 .. 2^31 - 1, got %u", n_assets_b);
    for (uint32_t i = 1; i < n_assets_a; ++i)
        if (asset_keys_a[i] <= asset_keys_a[i - 1])
            return fail(-EINVAL, "asset_keys_a must be strictly ascending: asset_keys_a[%u] <= asset_keys_a[%u]", i, i - 1);
    for (uint32_t i = 1; i < n_assets_b; ++i)
        if (asset_keys_b[i] <= asset_keys_b[i - 1])
            return fail(-EINVAL, "asset_keys_b must be strictly ascending: asset_keys_b[%u] <= asset_keys_b[%u]", i, i - 1);
    if (max_hamming < 0) return fail(-EINVAL, "max_hamming must be >= 0, got %d", max_hamming);
    if (max_doc_freq > 0 && max_doc_freq > dup_limit)
        return fail(-EINVAL, "max_doc_freq %u exceeds dup_limit %u: the frequency column counts no further", max_doc_freq, dup_limit);
    if (capacity >= (1ull << 31))
        return fail(-E2BIG, "capacity %llu: the two hits of a chunk pair are numbered with 32 bits", (unsigned long long)capacity);
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tabs[2];
    int rc;
    if ((rc = get_table(h, table_a, tabs[0]))) return rc;
    if ((rc = get_table(h, table_b, tabs[1]))) return rc;
    const uint32_t ids[2] = {table_a, table_b};
    for (int x = 0; x < 2; ++x)
        if (tabs[x]->metric != ISCCSEARCH_METRIC_HAMMING || tabs[x]->key_words != 2)
            return fail(-EINVAL, "join_overlaps_between needs simprint tables (HAMMING, key_words 2), table %u has metric %d and key_words %d", ids[x],
                        tabs[x]->metric, tabs[x]->key_words);
    if (tabs[0]->max_bytes != tabs[1]->max_bytes)
        return fail(-EINVAL, "simprint tables %u and %u hold codes of different lengths (max_bytes %d, %d)", table_a, table_b, tabs[0]->max_bytes, tabs[1]->max_bytes);
    const uint32_t nbytes = (uint32_t)tabs[0]->max_bytes;
    Segment* const segs[2] = {&tabs[0]->seg[nbytes], &tabs[1]->seg[nbytes]};
    for (int x = 0; x < 2; ++x)
        if (segs[x]->n >= (1ull << 32))
            return fail(-E2BIG, "a segment of %llu rows in table %u: row numbers travel as 32 bits", (unsigned long long)segs[x]->n, ids[x]);
    HIPOK(hipSetDevice(h->device));
    // the call's counters {chunk pairs, live rows a, stop chunks a, live rows b, stop chunks b, records}; per side (A first, B behind it)
    // asset keys, chunks per asset, row labels; the hits and records of isccsearch_join_overlaps for m = 2 * capacity
    const uint32_t n_assets[2] = {n_assets_a, n_assets_b};
    const uint64_t* const asset_keys[2] = {asset_keys_a, asset_keys_b};
    const uint64_t all_assets = (uint64_t)n_assets_a + n_assets_b, all_rows = segs[0]->n + segs[1]->n;
    const uint64_t m = 2 * capacity;
    size_t temp_bytes = 0;
    if ((rc = h->d_join_total.ensure(6))) return rc;
    if ((rc = h->d_join_live_keys.ensure(all_assets))) return rc;
    if ((rc = h->d_ov_chunks.ensure(all_assets))) return rc;
    if ((rc = h->d_join_row_labels.ensure(std::max<uint64_t>(all_rows, 1)))) return rc;
    if (m) {
        std::string err;
        if ((rc = iskov::aggregate_temp_bytes(m, &temp_bytes, &err))) return fail(rc, "%s", err.c_str());
        if ((rc = h->d_ov_hits.ensure(2 * m))) return rc;
        if ((rc = h->d_ov_marks.ensure(m))) return rc;
        if ((rc = h->d_ov_records.ensure(m))) return rc;
        if ((rc = h->d_ov_temp.ensure(std::max<size_t>(temp_bytes, 1)))) return rc;
    }
    // (each frequency column is built by a call of its own that drains the stream: nothing of this call is queued yet)
    for (int x = 0; x < 2; ++x)
        if (max_doc_freq > 0 && segs[x]->n && (rc = ensure_freq_column(h, *tabs[x], *segs[x], dup_limit))) return rc;
    unsigned long long* const counters = reinterpret_cast<unsigned long long*>(h->d_join_total.p);
    HIPOK(hipMemsetAsync(counters, 0, 6 * 8, h->stream));
    HIPOK(hipMemsetAsync(h->d_ov_chunks.p, 0, (size_t)all_assets * 4, h->stream));
    const bool launch = segs[0]->n && segs[1]->n;
    if (m && launch) HIPOK(hipMemsetAsync(h->d_ov_hits.p, 0xFF, m * sizeof(iskov::Hit), h->stream));
    uint32_t* row_labels[2] = {h->d_join_row_labels.p, h->d_join_row_labels.p + segs[0]->n};
    for (int x = 0; x < 2; ++x) {
        uint64_t* const d_keys = h->d_join_live_keys.p + (x ? n_assets_a : 0);
        HIPOK(hipMemcpyAsync(d_keys, asset_keys[x], (size_t)n_assets[x] * 8, hipMemcpyHostToDevice, h->stream));
        const Segment& s = *segs[x];
        if (!s.n) continue;
        // (label_chunks_kernel adds to counters[1] and [2] of the pointer it is given: table B's pair lies two further)
        isk::OverlapLabelParams lp{s.keys, d_keys, max_doc_freq > 0 ? s.freq : nullptr, row_labels[x], h->d_ov_chunks.p + (x ? n_assets_a : 0),
                                   counters + 2 * x, s.n, n_assets[x], max_doc_freq, x ? isk::LABEL_SIDE_B : 0u};
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((s.n + isk::BLOCK - 1) / isk::BLOCK, 1u << 16);
        hipLaunchKernelGGL(isk::label_chunks_kernel, dim3(blocks), dim3(isk::BLOCK), 0, h->stream, lp);
        HIPOK(hipGetLastError());
    }
    if (launch) {
        JoinPlan plan;
        plan.cross = true;
        plan.overlap = true;
        plan.KW = 2;
        plan.capacity = capacity;
        // as in isccsearch_join_between the segment with more rows is held: JoinEmit::labels_a are the HELD segment's labels
        const int held = segs[1]->n > segs[0]->n ? 1 : 0;
        if ((rc = join_add(h, plan, *segs[held], *segs[1 - held], nbytes, max_hamming, false, held == 1))) return rc;
        isk::JoinEmit& e = plan.emits.back();
        e.out_keys_a = e.out_keys_b = nullptr;        // the pair form's outputs: not this form's
        e.out_hamming = nullptr;
        e.out_prefix_bits = nullptr;
        e.labels_a = row_labels[held];
        e.labels_b = row_labels[1 - held];
        e.out_hits = reinterpret_cast<uint4*>(h->d_ov_hits.p);
        e.skip_same_key = flags & ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET ? 1u : 0u;
        if ((rc = join_run(h, plan))) return rc;
        if (m) {
            std::string err;
            if ((rc = iskov::aggregate(h->d_ov_hits.p, h->d_ov_hits.p + m, h->d_ov_marks.p, h->d_ov_records.p, counters + 5, m, h->d_ov_temp.p,
                                       temp_bytes, h->stream, &err)))
                return fail(rc, "%s", err.c_str());
        }
    }
    // the call's one synchronisation; the outputs change only from here on
    uint64_t got[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> chunks(all_assets);
    HIPOK(hipMemcpyAsync(got, counters, sizeof got, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(chunks.data(), h->d_ov_chunks.p, (size_t)all_assets * 4, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    const uint64_t total = got[0];
    if (total > capacity) {
        out_info[0] = total;
        return fail(-ENOSPC, "%llu chunk pairs do not fit the capacity of %llu", (unsigned long long)total, (unsigned long long)capacity);
    }
    // (slots were left unused: the run of ones behind the hits reduced to one more record, the last)
    const uint64_t n_records = m && launch ? got[5] - (total < capacity ? 1 : 0) : 0;
    if (n_records) {
        HIPOK(hipMemcpyAsync(out_pairs, h->d_ov_records.p, n_records * sizeof(isccsearch_overlap), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        // the side bit of src becomes the direction; the order by (src, dst) with the bit is the order by (reserved, src, dst) without
        for (uint64_t r = 0; r < n_records; ++r) {
            isccsearch_overlap& o = out_pairs[r];
            o.reserved = o.src >> 31;
            o.src &= ~isk::LABEL_SIDE_B;
            o.dst &= ~isk::LABEL_SIDE_B;
        }
    }
    memcpy(out_chunks_a, chunks.data(), (size_t)n_assets_a * 4);
    memcpy(out_chunks_b, chunks.data() + n_assets_a, (size_t)n_assets_b * 4);
    out_info[0] = total; out_info[1] = n_records; out_info[2] = got[1]; out_info[3] = got[2]; out_info[4] = got[3]; out_info[5] = got[4];
    return 0;
}
