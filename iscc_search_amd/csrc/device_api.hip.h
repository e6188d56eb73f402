// device_api.hip.h -- searches whose results stay on the device, the merges of such lists and the asynchronous search.
// Needs Batch, unpack_records, the query checks of isccsearch.hip, get_table of store.hip.h.
namespace {
// the queries of a device search, checked: they have ONE byte length (nothing is regrouped by length as in search_locked)
int one_query_length(const Table& t, uint32_t nq, const uint8_t* q_nbytes, uint32_t& len) {
    if (int rc = check_query_lengths(t, nq, q_nbytes)) return rc;
    len = t.metric == ISCCSEARCH_METRIC_NPHD ? q_nbytes[0] : (uint32_t)t.max_bytes;
    const uint32_t q = first_other_length(t, nq, q_nbytes);
    if (q < nq) return fail(-EINVAL, "search_device needs queries of one byte length (query %u differs)", q);
    return 0;
}

// lists produced on the caller's stream: order the library's stream behind it without a host round-trip
// (a caller that issued them on the library's own stream -- isccsearch_stream -- is ordered already)
int wait_for_producer(H* h, void* producer_stream) {
    if (static_cast<hipStream_t>(producer_stream) != h->stream) {
        HIPOK(hipEventRecord(h->ev_producer, static_cast<hipStream_t>(producer_stream)));
        HIPOK(hipStreamWaitEvent(h->stream, h->ev_producer, 0));
    }
    return 0;
}

int search_device_impl(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                       const uint8_t* q_nbytes, uint32_t k, int radius, void* d_records, uint32_t* d_counts) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (int rc = check_count(k)) return rc;
    if (radius > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", radius);
    if (nq == 0) return 0;
    if (!q_words || !d_records || !d_counts) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    uint32_t len;
    if ((rc = one_query_length(t, nq, q_nbytes, len))) return rc;
    HIPOK(hipSetDevice(h->device));
    h->stats.searches += 1;
    h->stats.queries += nq;
    isk::Record* out = static_cast<isk::Record*>(d_records);
    for (uint32_t pos = 0; pos < nq; pos += QB_MAX) {
        const uint32_t m = std::min<uint32_t>(QB_MAX, nq - pos);
        Batch batch(h, t, m, len, k, out + (size_t)pos * k, d_counts + pos);
        batch.radius = radius;
        const uint64_t* const hq = q_words + (size_t)pos * t.max_words;
        if ((rc = batch.begin(hq))) return rc;
        if ((rc = batch.finish(hq))) return rc;
    }
    HIPOK(hipStreamSynchronize(h->stream));
    return 0;
}

int merge_device_impl(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                      const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                      void* producer_stream, bool ordered,
                      uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (nq == 0) return 0;
    if (n_lists < 1 || k < 1 || k > ISCCSEARCH_MAX_K || (key_words != 1 && key_words != 2)) return fail(-EINVAL, "bad arguments");
    if (!d_records || !d_counts || !out_keys || !out_hamming || !out_prefix_bits || !out_count) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    int rc;
    if (list_stride % 8 || count_stride % 4 || (uintptr_t)d_records % 8 || (uintptr_t)d_counts % 4) return fail(-EINVAL, "misaligned record/count blocks");
    if (ordered && (rc = wait_for_producer(h, producer_stream))) return rc;
    // The merge writes its {records | counts} straight into ONE pinned host block (page-locked memory is mapped into the
    // device's address space): 240 bytes per query cross PCIe as the kernel's own stores, and the host needs a single
    // synchronisation -- no device->host copies to launch (each cost ~25 us of queue hand-over after the kernel).
    // (Blocks above DIRECT_RESULT_BYTES -- large k x many queries -- go through device memory and two DMA copies as before.)
    const ResultBlock blk = ResultBlock::merged(nq, k);
    const bool direct = blk.bytes() <= DIRECT_RESULT_BYTES;
    if ((rc = h->p_block.ensure(blk.bytes()))) return rc;
    if (!direct) {
        if ((rc = h->d_final.ensure((size_t)nq * k))) return rc;
        if ((rc = h->d_outcnt.ensure(nq))) return rc;
    }
    isk::MergeParams mp{static_cast<const unsigned char*>(d_records), static_cast<const unsigned char*>(d_counts),
                        list_stride, count_stride,
                        direct ? blk.records(h->p_block.p) : h->d_final.p, direct ? blk.counts(h->p_block.p) : h->d_outcnt.p, n_lists, nq, k};
    hipLaunchKernelGGL(isk::merge_kernel, dim3(nq), dim3(isk::BLOCK), 0, h->stream, mp);
    HIPOK(hipGetLastError());
    if (!direct) {
        HIPOK(hipMemcpyAsync(blk.records(h->p_block.p), h->d_final.p, blk.records_bytes(), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipMemcpyAsync(blk.counts(h->p_block.p), h->d_outcnt.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPOK(hipStreamSynchronize(h->stream));
    unpack_records(blk.records(h->p_block.p), blk.counts(h->p_block.p), nq, k, key_words, nullptr, out_keys, out_hamming, out_prefix_bits, out_count);
    return 0;
}
}  // namespace

extern "C" {
int isccsearch_search_device(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                             const uint8_t* q_nbytes, uint32_t k, void* d_records, uint32_t* d_counts) {
    return search_device_impl(h, table, nq, q_words, q_nbytes, k, -1, d_records, d_counts);
}

int isccsearch_search_within_device(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                    const uint8_t* q_nbytes, uint32_t k, uint32_t max_hamming,
                                    void* d_records, uint32_t* d_counts) {
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %u exceeds 256", max_hamming);
    return search_device_impl(h, table, nq, q_words, q_nbytes, k, (int)max_hamming, d_records, d_counts);
}

int isccsearch_merge_device(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                            const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                            uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    return merge_device_impl(h, n_lists, nq, k, key_words, d_records, d_counts, list_stride, count_stride, nullptr, false,
                             out_keys, out_hamming, out_prefix_bits, out_count);
}

int isccsearch_merge_device_after(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                                  const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                                  void* producer_stream,
                                  uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    return merge_device_impl(h, n_lists, nq, k, key_words, d_records, d_counts, list_stride, count_stride, producer_stream, true,
                             out_keys, out_hamming, out_prefix_bits, out_count);
}

// Several merges behind ONE synchronisation: the per-unit searches of one request on a sharded index share one all-gather
// (sharded.py, ShardedTable.search_many); their merges are queued back to back into distinct parts of the pinned result block
// and read after a single hipStreamSynchronize (each merge_device_after call costs one: ~50 us per unit).
int isccsearch_merge_many_after(isccsearch_handle* h, uint32_t n, isccsearch_merge_request* reqs, void* producer_stream) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!reqs) return fail(-EINVAL, "NULL argument");
    size_t total = 0;
    std::vector<size_t> off(n);
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_merge_request& r = reqs[i];
        if (r.nq == 0 || r.n_lists < 1 || r.k < 1 || r.k > ISCCSEARCH_MAX_K || (r.key_words != 1 && r.key_words != 2)) return fail(-EINVAL, "bad arguments (merge %u)", i);
        if (!r.d_records || !r.d_counts || !r.out_keys || !r.out_hamming || !r.out_prefix_bits || !r.out_count) return fail(-EINVAL, "NULL argument (merge %u)", i);
        if (r.list_stride % 8 || r.count_stride % 4 || (uintptr_t)r.d_records % 8 || (uintptr_t)r.d_counts % 4) return fail(-EINVAL, "misaligned record/count blocks (merge %u)", i);
        off[i] = total;
        total += ResultBlock::merged(r.nq, r.k).slice_bytes();
    }
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    int rc;
    // the kernels write their {records | counts} straight into the pinned block (mapped into the device's address space); a request
    // whose results do not fit the direct budget goes through the ordinary call
    if (total > DIRECT_RESULT_BYTES) return fail(-E2BIG, "merge_many: %zu bytes of results exceed the directly written block", total);
    if ((rc = h->p_block.ensure(total))) return rc;
    if ((rc = wait_for_producer(h, producer_stream))) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_merge_request& r = reqs[i];
        const ResultBlock blk = ResultBlock::merged(r.nq, r.k);
        isk::MergeParams mp{static_cast<const unsigned char*>(r.d_records), static_cast<const unsigned char*>(r.d_counts), r.list_stride, r.count_stride,
                            blk.records(h->p_block.p + off[i]), blk.counts(h->p_block.p + off[i]), r.n_lists, r.nq, r.k};
        hipLaunchKernelGGL(isk::merge_kernel, dim3(r.nq), dim3(isk::BLOCK), 0, h->stream, mp);
    }
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_merge_request& r = reqs[i];
        const ResultBlock blk = ResultBlock::merged(r.nq, r.k);
        unpack_records(blk.records(h->p_block.p + off[i]), blk.counts(h->p_block.p + off[i]), r.nq, r.k, r.key_words,
                       nullptr, r.out_keys, r.out_hamming, r.out_prefix_bits, r.out_count);
    }
    return 0;
}

int isccsearch_search_device_async(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                   const uint8_t* q_nbytes, uint32_t k, int32_t max_hamming,
                                   void* d_records, uint32_t* d_counts, void* consumer_stream) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", max_hamming);
    const int radius = max_hamming < 0 ? -1 : max_hamming;
    bool async = nq > 0 && nq <= QB_MAX && k >= 1 && k <= ISCCSEARCH_MAX_K && q_words && d_records && d_counts;
    // the one-shot hint belongs to THIS call whatever becomes of it: read and clear it before anything can return (an early
    // return used to leave it armed for the next, unrelated call, whose caller would not verify its lists)
    int hint;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        hint = (int)h->opt.device_search_hint;
        h->opt.device_search_hint = -1;
    }
    if (async) {
        std::lock_guard<std::mutex> lk(h->mu);
        Table* tp;
        int rc = get_table(h, table, tp);
        if (rc) return rc;
        Table& t = *tp;
        uint32_t len;
        if ((rc = one_query_length(t, nq, q_nbytes, len))) return rc;
        if (t.segments() <= 1) {
            HIPOK(hipSetDevice(h->device));
            h->stats.searches += 1;
            h->stats.queries += nq;
            Batch batch(h, t, nq, len, k, static_cast<isk::Record*>(d_records), d_counts);
            batch.radius = radius;
            batch.mark_overflow = true;
            // (sharded callers: the GLOBAL k-th distance of the previous step + margin -- every shard then lists its rows under it,
            //  tightening as it finds k of its own, and the caller accepts the merged lists only if they hold k rows per query)
            // ... a SMALL batch (the protocol's per-unit searches on a sharded index) takes the hint as the radius of one range-limited
            // pass -- radius_init + collect + select instead of bootstrap + levels + picks + collect -- as search_locked's speculative
            // pass does on one GPU; same contract: the table's nearest rows within the hint, fewer than k if it was too tight
            if (radius < 0 && hint >= 0) {
                if (h->opt.speculate && nq <= (uint32_t)h->opt.spec_max_queries) batch.radius = hint;
                else batch.self_hint = hint;
            }
            if ((rc = batch.begin(q_words))) return rc;
            if (static_cast<hipStream_t>(consumer_stream) != h->stream) {
                HIPOK(hipEventRecord(h->ev_done, h->stream));
                HIPOK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), h->ev_done, 0));
            }
            return 0;
        }
    }
    // several segments (their lists must be fixed and merged with the host's help), oversized batches, bad arguments: the
    // synchronous path does the work and the reporting; the results are complete when it returns
    return search_device_impl(h, table, nq, q_words, q_nbytes, k, radius, d_records, d_counts);
}
}  // extern "C"
