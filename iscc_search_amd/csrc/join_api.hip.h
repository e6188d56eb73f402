// join_api.hip.h -- isccsearch_join_within: the self-join of a table by the kernel of join.hip.h.
// Needs the store of isccsearch.hip (Segment, Table; get_table of store.hip.h) and its scratch buffers.
namespace {
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

// One join_scan_kernel launch per pair of segments (join.hip.h), all appending to one output; the pairs are sorted on the host.
extern "C" int isccsearch_join_within(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t capacity,
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
            set_cols(L.jp.col_a, A, W);
            set_cols(L.jp.col_b, B, W);
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
