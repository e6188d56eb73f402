// store.hip.h -- the column store: handle creation / destruction / options / statistics, tables, segments, the lazy key index and
// the add / remove / get / export entry points.  Needs the common part of isccsearch.hip, and drain_events of its pipeline.
namespace {
void build_rank_table(std::vector<uint16_t>& rank) {
    // rank[p][h] for p in 1..32 bytes: position of h/(8p) among all distinct fractions; row 0: identity
    struct Fr { uint32_t h, p; };
    std::vector<Fr> all;
    for (uint32_t p = 1; p <= 32; ++p)
        for (uint32_t h = 0; h <= 8 * p; ++h) all.push_back({h, p});
    auto less = [](const Fr& a, const Fr& b) { return (uint64_t)a.h * b.p < (uint64_t)b.h * a.p; };
    std::sort(all.begin(), all.end(), less);
    rank.assign(33 * 257, 0xFFFF);
    uint32_t r = 0;
    for (size_t i = 0; i < all.size(); ++i) {
        if (i && less(all[i - 1], all[i])) ++r;
        rank[all[i].p * 257 + all[i].h] = (uint16_t)r;
    }
    for (uint32_t h = 0; h <= 256; ++h) rank[h] = (uint16_t)h;
}

int seg_reserve(H* h, Table& t, Segment& s, uint64_t need) {
    if (need <= s.cap) return 0;
    uint64_t cap = std::max<uint64_t>(need, s.cap * 2);
    cap = (cap + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
    uint64_t* ncol[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t* nkeys = nullptr;
    auto cleanup = [&]() { for (auto& c : ncol) if (c) (void)hipFree(c); if (nkeys) (void)hipFree(nkeys); };
    for (uint32_t w = 0; w < s.W; ++w) {
        hipError_t e = hipMalloc((void**)&ncol[w], cap * 8);
        if (e != hipSuccess) { cleanup(); (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(column, %llu bytes) failed: %s", (unsigned long long)cap * 8, hipGetErrorString(e)); }
    }
    {
        hipError_t e = hipMalloc((void**)&nkeys, cap * 8 * t.key_words);
        if (e != hipSuccess) { cleanup(); (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(keys) failed: %s", hipGetErrorString(e)); }
    }
    if (s.n) {
        // a failure here must not leak the new columns (the old ones stay in place and valid)
        hipError_t e = hipSuccess;
        for (uint32_t w = 0; w < s.W && e == hipSuccess; ++w) e = hipMemcpyAsync(ncol[w], s.col[w], s.n * 8, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nkeys, s.keys, s.n * 8 * t.key_words, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            cleanup();
            (void)hipGetLastError();
            return fail(-EIO, "growing a segment to %llu rows failed while copying: %s", (unsigned long long)cap, hipGetErrorString(e));
        }
    }
    for (uint32_t w = 0; w < s.W; ++w) { if (s.col[w]) (void)hipFree(s.col[w]); s.col[w] = ncol[w]; }
    if (s.keys) (void)hipFree(s.keys);
    s.keys = nkeys;
    s.cap = cap;
    return 0;
}

int get_table(H* h, uint32_t id, Table*& out) {
    if (id >= h->tables.size() || !h->tables[id] || !h->tables[id]->open) return fail(-ENOENT, "table %u is not open", id);
    out = h->tables[id].get();
    return 0;
}

// key i of an array of keys (KW words each; two words are hi, lo)
Key key_at(const uint64_t* keys, uint64_t i, int KW) { return KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]}; }

int ensure_index(H* h, Table& t) {
    if (t.indexed) return 0;
    t.index.reset(t.key_words == 2);
    t.index.reserve((size_t)t.total + 16);
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        Segment& s = t.seg[b];
        if (!s.n) { s.hkeys.clear(); continue; }
        s.hkeys.resize((size_t)s.n * t.key_words);
        HIPOK(hipMemcpyAsync(s.hkeys.data(), s.keys, s.n * 8 * t.key_words, hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (uint64_t r = 0; r < s.n; ++r) t.index.set(key_at(s.hkeys.data(), r, t.key_words), Loc{b, r});
    }
    t.indexed = true;
    return 0;
}

// rows that are not trusted to be new: none of the n keys may be in the table already, or twice in the batch
int check_new_keys(H* h, Table& t, uint64_t n, const uint64_t* keys) {
    int rc;
    if ((rc = ensure_index(h, t))) return rc;
    std::unordered_map<Key, int, KeyHash> seen;
    seen.reserve((size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        const Key k = key_at(keys, i, t.key_words);
        if (t.index.contains(k) || !seen.emplace(k, 1).second)
            return fail(-EEXIST, "key %016llx%016llx already present (row %llu of the batch)", (unsigned long long)k.hi, (unsigned long long)k.lo, (unsigned long long)i);
    }
    return 0;
}

// m rows have been written behind segment s's last: the host mirror of the keys and the index follow when the table is indexed
// (`keys`, the new rows' keys, is read only then), and the row counts -- Table::total stays the sum of its segments' rows
void commit_rows(Table& t, Segment& s, const uint64_t* keys, uint64_t m) {
    if (t.indexed) {
        s.hkeys.insert(s.hkeys.end(), keys, keys + m * t.key_words);
        for (uint64_t r = 0; r < m; ++r) t.index.set(key_at(keys, r, t.key_words), Loc{s.nbytes, s.n + r});
    }
    s.n += m; s.touch(); t.total += m;
}

// the code length of a segment named by the caller; `stored`: rows of that length can be stored (a Hamming table has one length only)
int check_nbytes(const Table& t, int nbytes, bool stored = true) {
    if (nbytes < 1 || nbytes > t.max_bytes) return fail(-EINVAL, "nbytes %d outside 1..%d", nbytes, t.max_bytes);
    if (stored && t.metric == ISCCSEARCH_METRIC_HAMMING && nbytes != t.max_bytes) return fail(-EINVAL, "Hamming tables hold %d-byte codes only", t.max_bytes);
    return 0;
}

// the keys that are present, through the index: per segment their rows and, alongside, their positions in the call
// (out_nbytes, when given, takes the code length of every key found)
void locate_rows(const Table& t, uint64_t n, const uint64_t* keys, std::vector<uint64_t>* rows, std::vector<uint64_t>* dest, uint8_t* out_nbytes = nullptr) {
    for (uint64_t i = 0; i < n; ++i) {
        Loc loc;
        if (!t.index.find(key_at(keys, i, t.key_words), loc)) continue;
        rows[loc.seg].push_back(loc.row);
        dest[loc.seg].push_back(i);
        if (out_nbytes) out_nbytes[i] = (uint8_t)loc.seg;
    }
}

// the segment's document-frequency column (docfreq.hip), (re)built when rows changed since it was made
int ensure_freq_column(H* h, Table& t, Segment& s, uint32_t dup_limit) {
    if (s.freq_rows == s.n && s.freq_dup == dup_limit && s.freq) return 0;
    if (s.freq) { (void)hipFree(s.freq); s.freq = nullptr; }
    s.freq_rows = 0;
    hipError_t e = hipMalloc((void**)&s.freq, s.n * sizeof(uint32_t));
    if (e != hipSuccess) { s.freq = nullptr; (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(frequency column, %llu bytes) failed: %s", (unsigned long long)s.n * 4, hipGetErrorString(e)); }
    std::string err;
    int rc;
    if ((rc = iskdf::build_freq_column(s.col, (int)s.W, s.keys, t.key_words, s.n, dup_limit, s.freq, h->stream, &err))) return fail(rc, "%s", err.c_str());
    s.freq_rows = s.n;
    s.freq_dup = dup_limit;
    h->stats.freq_builds += 1;
    return 0;
}
}  // namespace

extern "C" {
const char* isccsearch_last_error(void) { return g_last_error.c_str(); }

int isccsearch_create(int device_id, isccsearch_handle** out) {
    if (!out) return fail(-EINVAL, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(-ENODEV, "no HIP device available (%s)", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(-ENODEV, "device %d out of range (0..%d)", device_id, ndev - 1);
    HIPOK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPOK(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(-ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
    std::unique_ptr<isccsearch_handle> h(new isccsearch_handle());
    h->device = device_id;
    h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIPOK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPOK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&h->ev_staged, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&h->ev_producer, hipEventDisableTiming));
    std::vector<uint16_t> rank;
    build_rank_table(rank);
    HIPOK(hipMalloc((void**)&h->d_rank, rank.size() * sizeof(uint16_t)));
    HIPOK(hipMemcpy(h->d_rank, rank.data(), rank.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    // the select kernel may need more than the default dynamic LDS for k near ISCCSEARCH_MAX_K
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    h->stats.queries_per_pass = (uint32_t)h->opt.queries_per_pass;
    h->stats.compute_units = h->cus;
    *out = h.release();
    return 0;
}

void* isccsearch_stream(isccsearch_handle* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

int isccsearch_destroy(isccsearch_handle* h) {
    if (!h) return 0;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        h->teardown();
    }
    delete h;     // (the mutex is released before the handle that owns it goes)
    return 0;
}

// (both walk OPTIONS, the one list of what can be set and read)
int isccsearch_set_option(isccsearch_handle* h, const char* name, int64_t value) {
    if (!h || !name) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    const OptionDesc* d = find_option(name);
    if (!d) return fail(-EINVAL, "unknown option '%s'", name);
    // queries_per_pass: 32 is not offered (its query registers spill to scratch, which the asm-issued loads forbid), nor anything between
    if (d->field == &Options::queries_per_pass && value != 8 && value != 16) return fail(-EINVAL, "queries_per_pass must be 8 or 16");
    if (value < d->min || value > d->max)
        return d->max == NO_MAX ? fail(-EINVAL, "%s must be >= %lld", name, (long long)d->min)
                                : fail(-EINVAL, "%s must be %lld..%lld", name, (long long)d->min, (long long)d->max);
    h->opt.*(d->field) = value;
    h->stats.queries_per_pass = (uint32_t)h->opt.queries_per_pass;
    return 0;
}

int isccsearch_get_option(isccsearch_handle* h, const char* name, int64_t* value) {
    if (!h || !name || !value) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    const OptionDesc* d = find_option(name);
    if (!d) return fail(-EINVAL, "unknown option '%s'", name);
    *value = h->opt.*(d->field);
    return 0;
}

int isccsearch_stats_get(isccsearch_handle* h, isccsearch_stats* out, int reset) {
    if (!h || !out) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    int rc = drain_events(h);
    if (rc) return rc;
    *out = h->stats;
    if (reset) {
        const uint32_t tq = h->stats.queries_per_pass, cu = h->stats.compute_units;
        h->stats = isccsearch_stats{};
        h->stats.queries_per_pass = tq;
        h->stats.compute_units = cu;
    }
    return 0;
}

int isccsearch_table_open(isccsearch_handle* h, int metric, int key_words, int max_bytes, uint32_t* table_id) {
    if (!h || !table_id) return fail(-EINVAL, "bad arguments");
    if (metric != ISCCSEARCH_METRIC_HAMMING && metric != ISCCSEARCH_METRIC_NPHD) return fail(-EINVAL, "unknown metric %d", metric);
    if (key_words != 1 && key_words != 2) return fail(-EINVAL, "key_words must be 1 or 2");
    if (max_bytes < 1 || max_bytes > ISCCSEARCH_MAX_BYTES) return fail(-EINVAL, "max_bytes must be 1..%d", ISCCSEARCH_MAX_BYTES);
    std::lock_guard<std::mutex> lk(h->mu);
    std::unique_ptr<Table> t(new Table());
    t->open = true;
    t->metric = metric;
    t->key_words = key_words;
    t->max_bytes = max_bytes;
    t->max_words = (max_bytes + 7) / 8;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) { t->seg[b].nbytes = b; t->seg[b].W = (b + 7) / 8; }
    for (size_t i = 0; i < h->tables.size(); ++i)
        if (!h->tables[i]) { h->tables[i] = std::move(t); *table_id = (uint32_t)i; return 0; }
    h->tables.push_back(std::move(t));
    *table_id = (uint32_t)(h->tables.size() - 1);
    return 0;
}

int isccsearch_table_drop(isccsearch_handle* h, uint32_t table) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* t;
    int rc = get_table(h, table, t);
    if (rc) return rc;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    for (auto& s : t->seg) seg_free(s);
    h->tables[table].reset();
    return 0;
}

int isccsearch_reserve(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t rows) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* t;
    int rc = get_table(h, table, t);
    if (rc) return rc;
    if ((rc = check_nbytes(*t, nbytes))) return rc;
    HIPOK(hipSetDevice(h->device));
    return seg_reserve(h, *t, t->seg[nbytes], rows);
}

uint64_t isccsearch_size(isccsearch_handle* h, uint32_t table) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    Table* t;
    if (get_table(h, table, t)) return 0;
    return t->total;
}

int isccsearch_add(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                   const uint64_t* code_words, const uint8_t* nbytes, uint32_t flags) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !code_words) return fail(-EINVAL, "keys/code_words are NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    const int KW = t.key_words, MW = t.max_words;
    if (t.metric == ISCCSEARCH_METRIC_NPHD && !nbytes) return fail(-EINVAL, "nbytes is required for NPHD tables");
    // validate lengths, count rows per segment
    uint64_t per_seg[ISCCSEARCH_MAX_BYTES + 1] = {0};
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t b = nbytes ? nbytes[i] : (uint32_t)t.max_bytes;
        if (b < 1 || b > (uint32_t)t.max_bytes) return fail(-EINVAL, "row %llu: code length %u outside 1..%d bytes", (unsigned long long)i, b, t.max_bytes);
        if (t.metric == ISCCSEARCH_METRIC_HAMMING && b != (uint32_t)t.max_bytes) return fail(-EINVAL, "row %llu: Hamming table holds %d-byte codes, got %u", (unsigned long long)i, t.max_bytes, b);
        per_seg[b]++;
    }
    if (!(flags & ISCCSEARCH_ADD_TRUSTED_UNIQUE) && (rc = check_new_keys(h, t, n, keys))) return rc;
    // grow segments
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b)
        if (per_seg[b] && (rc = seg_reserve(h, t, t.seg[b], t.seg[b].n + per_seg[b]))) return rc;
    // stage per segment (word-major) and copy
    std::vector<uint64_t> stage, kstage;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        const uint64_t m = per_seg[b];
        if (!m) continue;
        Segment& s = t.seg[b];
        // single segment, one whole word: the caller's buffers are already column-shaped (shorter one-word codes take the split below,
        // which masks the bits past their length)
        const bool direct = (m == n && MW == 1 && b == 8);
        const uint64_t* kp = keys;
        if (direct) {
            HIPOK(hipMemcpyAsync(s.col[0] + s.n, code_words, m * 8, hipMemcpyHostToDevice, h->stream));
        } else if (m == n) {
            // one code length, several words or a masked one: ship the caller's row-major block as it is and split it into the
            // word columns on the device (a host-side transposition capped 256-bit ingest at 80 M rows/s)
            if ((rc = h->d_misc2.ensure((size_t)n * MW))) return rc;
            HIPOK(hipMemcpyAsync(h->d_misc2.p, code_words, (size_t)n * MW * 8, hipMemcpyHostToDevice, h->stream));
            isk::SplitParams sp{};
            set_cols(sp.col, s, s.W);
            sp.rows = h->d_misc2.p; sp.dst_row = s.n; sp.n = n; sp.W = s.W; sp.MW = (uint32_t)MW; sp.mask_last = mask_for(b);
            const uint32_t grid = (uint32_t)std::min<uint64_t>((n + isk::BLOCK - 1) / isk::BLOCK, (uint64_t)h->cus * 8);
            hipLaunchKernelGGL(isk::split_rows_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, sp);
            HIPOK(hipGetLastError());
        } else {
            stage.resize((size_t)m * s.W);
            uint64_t j = 0;
            const uint64_t lastmask = mask_for(b);
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t bi = nbytes ? nbytes[i] : (uint32_t)t.max_bytes;
                if (bi != b) continue;
                for (uint32_t w = 0; w < s.W; ++w) {
                    uint64_t v = code_words[i * MW + w];
                    if (w == s.W - 1) v &= lastmask;
                    stage[(size_t)w * m + j] = v;
                }
                ++j;
            }
            for (uint32_t w = 0; w < s.W; ++w)
                HIPOK(hipMemcpyAsync(s.col[w] + s.n, stage.data() + (size_t)w * m, m * 8, hipMemcpyHostToDevice, h->stream));
        }
        if (m != n) {
            kstage.resize((size_t)m * KW);
            uint64_t j = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t bi = nbytes ? nbytes[i] : (uint32_t)t.max_bytes;
                if (bi != b) continue;
                for (int w = 0; w < KW; ++w) kstage[(size_t)j * KW + w] = keys[i * KW + w];
                ++j;
            }
            kp = kstage.data();
        }
        HIPOK(hipMemcpyAsync(s.keys + s.n * KW, kp, m * 8 * KW, hipMemcpyHostToDevice, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        commit_rows(t, s, kp, m);
    }
    return 0;
}

int isccsearch_segments(isccsearch_handle* h, uint32_t table, uint64_t* out_rows) {
    if (!h || !out_rows) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    out_rows[0] = 0;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) out_rows[b] = tp->seg[b].n;
    return 0;
}

int isccsearch_export(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t first_row, uint64_t n,
                      uint64_t* out_keys, uint64_t* out_cols) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!out_keys || !out_cols) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    if ((rc = check_nbytes(*tp, nbytes, false))) return rc;
    Segment& s = tp->seg[nbytes];
    if (first_row > s.n || n > s.n - first_row) return fail(-EINVAL, "rows [%llu, +%llu) outside the segment's %llu rows", (unsigned long long)first_row, (unsigned long long)n, (unsigned long long)s.n);
    HIPOK(hipSetDevice(h->device));
    for (uint32_t w = 0; w < s.W; ++w)
        HIPOK(hipMemcpyAsync(out_cols + (size_t)w * n, s.col[w] + first_row, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(out_keys, s.keys + first_row * tp->key_words, n * 8 * tp->key_words, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    return 0;
}

int isccsearch_add_columns(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t n, const uint64_t* keys,
                           const uint64_t* cols, uint32_t flags) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !cols) return fail(-EINVAL, "keys/cols are NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if ((rc = check_nbytes(t, nbytes))) return rc;
    HIPOK(hipSetDevice(h->device));
    const int KW = t.key_words;
    if (!(flags & ISCCSEARCH_ADD_TRUSTED_UNIQUE) && (rc = check_new_keys(h, t, n, keys))) return rc;
    Segment& s = t.seg[nbytes];
    if ((rc = seg_reserve(h, t, s, s.n + n))) return rc;
    for (uint32_t w = 0; w < s.W; ++w)
        HIPOK(hipMemcpyAsync(s.col[w] + s.n, cols + (size_t)w * n, n * 8, hipMemcpyHostToDevice, h->stream));
    if (nbytes & 7) {
        // bits past the code length are stored as zero whatever the caller left there (whole-word codes have none)
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + isk::BLOCK - 1) / isk::BLOCK, (uint64_t)h->cus * 8);
        hipLaunchKernelGGL(isk::mask_column_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, s.col[s.W - 1] + s.n, n, mask_for((uint32_t)nbytes));
        HIPOK(hipGetLastError());
    }
    HIPOK(hipMemcpyAsync(s.keys + s.n * KW, keys, n * 8 * KW, hipMemcpyHostToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    commit_rows(t, s, keys, n);
    return 0;
}

int isccsearch_add_synthetic(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t n,
                             uint64_t seed, uint64_t first_row, uint64_t key_base) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if ((rc = check_nbytes(t, nbytes))) return rc;
    if (t.indexed) return fail(-EINVAL, "synthetic rows cannot be added to a table whose key index is built");
    HIPOK(hipSetDevice(h->device));
    Segment& s = t.seg[nbytes];
    if ((rc = seg_reserve(h, t, s, s.n + n))) return rc;
    isk::FillParams fp{};
    set_cols(fp.col, s, s.W);
    fp.keys = s.keys; fp.dst_row = s.n; fp.n = n; fp.seed = seed; fp.first_row = first_row; fp.key_base = key_base;
    fp.W = s.W; fp.KW = (uint32_t)t.key_words; fp.mask_last = mask_for((uint32_t)nbytes);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + isk::BLOCK - 1) / isk::BLOCK, (uint64_t)h->cus * 16);
    hipLaunchKernelGGL(isk::fill_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, fp);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(h->stream));
    commit_rows(t, s, nullptr, n);      // (never indexed, see above: no keys to mirror)
    return 0;
}

int isccsearch_remove(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys, uint64_t* n_removed) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n_removed) *n_removed = 0;
    if (n == 0) return 0;
    if (!keys) return fail(-EINVAL, "keys is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, t))) return rc;
    const int KW = t.key_words;
    // the host index is updated key by key below and the row moves are replayed on the device afterwards: reserve what that
    // replay needs BEFORE anything changes, so that an allocation failure cannot leave host and device rows disagreeing
    if ((rc = h->d_misc.ensure((size_t)n * 2))) return rc;
    std::vector<uint64_t> moves[ISCCSEARCH_MAX_BYTES + 1];
    uint64_t removed = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const Key k = key_at(keys, i, KW);
        Loc loc;
        if (!t.index.find(k, loc)) continue;
        Segment& s = t.seg[loc.seg];
        const uint64_t last = s.n - 1;
        t.index.erase(k);
        if (loc.row != last) {
            const Key lk2 = key_at(s.hkeys.data(), last, KW);
            for (int w = 0; w < KW; ++w) s.hkeys[loc.row * KW + w] = s.hkeys[last * KW + w];
            t.index.set(lk2, Loc{loc.seg, loc.row});
            moves[loc.seg].push_back(loc.row);
            moves[loc.seg].push_back(last);
        }
        s.hkeys.resize((size_t)last * KW);
        s.n = last;
        s.touch();
        t.total--;
        ++removed;
    }
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        if (moves[b].empty()) continue;
        Segment& s = t.seg[b];
        if ((rc = h->d_misc.ensure(moves[b].size()))) return rc;
        HIPOK(hipMemcpyAsync(h->d_misc.p, moves[b].data(), moves[b].size() * 8, hipMemcpyHostToDevice, h->stream));
        isk::MoveParams mp{};
        set_cols(mp.col, s, s.W);
        mp.keys = s.keys; mp.moves = h->d_misc.p; mp.n_moves = moves[b].size() / 2; mp.W = s.W; mp.KW = (uint32_t)KW;
        hipLaunchKernelGGL(isk::move_rows_kernel, dim3(1), dim3(64), 0, h->stream, mp);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(h->stream));
    }
    if (n_removed) *n_removed = removed;
    return 0;
}

int isccsearch_contains(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys, uint8_t* out_found) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !out_found) return fail(-EINVAL, "keys/out_found are NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, *tp))) return rc;
    const int KW = tp->key_words;
    for (uint64_t i = 0; i < n; ++i) out_found[i] = tp->index.contains(key_at(keys, i, KW)) ? 1 : 0;
    return 0;
}

int isccsearch_get(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                   uint64_t* out_words, uint8_t* out_nbytes) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !out_words || !out_nbytes) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, t))) return rc;
    const int MW = t.max_words;
    memset(out_words, 0, (size_t)n * MW * 8);
    memset(out_nbytes, 0, (size_t)n);
    std::vector<uint64_t> rows[ISCCSEARCH_MAX_BYTES + 1], dest[ISCCSEARCH_MAX_BYTES + 1];
    locate_rows(t, n, keys, rows, dest, out_nbytes);
    std::vector<uint64_t> tmp;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        if (rows[b].empty()) continue;
        Segment& s = t.seg[b];
        const uint64_t m = rows[b].size();
        if ((rc = h->d_misc.ensure(m))) return rc;
        if ((rc = h->d_misc2.ensure(m * s.W))) return rc;
        HIPOK(hipMemcpyAsync(h->d_misc.p, rows[b].data(), m * 8, hipMemcpyHostToDevice, h->stream));
        isk::GatherParams gp{};
        set_cols(gp.col, s, s.W);
        gp.rows = h->d_misc.p; gp.out = h->d_misc2.p; gp.n = m; gp.W = s.W;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((m + isk::BLOCK - 1) / isk::BLOCK, 1024);
        hipLaunchKernelGGL(isk::gather_rows_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, gp);
        HIPOK(hipGetLastError());
        tmp.resize(m * s.W);
        HIPOK(hipMemcpyAsync(tmp.data(), h->d_misc2.p, m * s.W * 8, hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (uint64_t i = 0; i < m; ++i)
            for (uint32_t w = 0; w < s.W; ++w) out_words[dest[b][i] * MW + w] = tmp[i * s.W + w];
    }
    return 0;
}

// freq[i] = document frequency of the code stored under keys[i] (0 when the key is absent), read from the
// segment's document-frequency column; the column is (re)built here when rows changed since it was made.
int isccsearch_get_freq(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                        uint32_t dup_limit, uint32_t* out_freq) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1) return fail(-EINVAL, "dup_limit must be >= 1");
    if (n == 0) return 0;
    if (!keys || !out_freq) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if (t.metric != ISCCSEARCH_METRIC_HAMMING) return fail(-EINVAL, "get_freq is defined for fixed-length (Hamming) tables");
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, t))) return rc;
    memset(out_freq, 0, (size_t)n * sizeof(uint32_t));
    std::vector<uint64_t> rows[ISCCSEARCH_MAX_BYTES + 1], dest[ISCCSEARCH_MAX_BYTES + 1];
    locate_rows(t, n, keys, rows, dest);
    std::vector<uint32_t> tmp;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        if (rows[b].empty()) continue;
        Segment& s = t.seg[b];
        if ((rc = ensure_freq_column(h, t, s, dup_limit))) return rc;
        const uint64_t m = rows[b].size();
        if ((rc = h->d_misc.ensure(m))) return rc;
        if ((rc = h->d_freq.ensure(m))) return rc;
        HIPOK(hipMemcpyAsync(h->d_misc.p, rows[b].data(), m * 8, hipMemcpyHostToDevice, h->stream));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((m + isk::BLOCK - 1) / isk::BLOCK, 1024);
        hipLaunchKernelGGL(isk::gather_u32_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, s.freq, h->d_misc.p, h->d_freq.p, m);
        HIPOK(hipGetLastError());
        tmp.resize(m);
        HIPOK(hipMemcpyAsync(tmp.data(), h->d_freq.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (uint64_t i = 0; i < m; ++i) out_freq[dest[b][i]] = tmp[i];
    }
    return 0;
}
}  // extern "C"
