// api_emit.hip — the C ABI of include/rass_engine.h: the searches that ride the exact fp32 scan and emit on the way, with
// no ranking: the score-threshold search rass_index_search_range(_device), the grouped (collapsed) search
// rass_index_search_grouped(_device) and the terms aggregation rass_index_aggregate(_device), and the last two over a caller's
// key column and bitmap: rass_index_search_grouped_keys(_device), rass_index_aggregate_keys(_device).  One device-group driver
// (emit_begin / emit_scan) serves them all; the host variants go through host_groups.  Host-side C++ only: the kernels are scan_topk.hip
// (ScanMode kRange / kGroupMax / kGroupCount / kGroupMaxKeys / kGroupCountKeys), merge_topk.hip and group_topk.hip.  The objects and the threading rules:
// api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// What the three requests share.  Everything is a device pointer.
struct EmitRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    // the key-column forms of the grouped search and the aggregation: the rows' groups (nullptr: a bit field of the tag) and
    // the bitmap(s) of THIS launch group's queries (nullptr: no restriction; allow_q_stride 0: one shared by all of them)
    const int32_t* keys = nullptr;
    int64_t n_keys = 0;
    const uint32_t* allow = nullptr;
    int64_t allow_q_stride = 0, allow_words = 0;
};

// What the caller of a key-column entry point passed, whole: key_request cuts out a launch group's part.
struct KeyArgs {
    const int32_t* keys;
    int64_t n_keys;
    const uint32_t* allow;
    int n_bitmaps;
    int64_t words;
};
constexpr int32_t kWholeKey = 0x7fffffff;   // group_mask of a key-column request: the whole (non-negative) key is the group

void key_request(EmitRequest& r, const KeyArgs* kv, int done) {
    if (!kv) return;
    r.keys = kv->keys, r.n_keys = kv->n_keys;
    if (kv->allow) {
        r.allow_q_stride = kv->n_bitmaps == 1 ? 0 : kv->words;
        r.allow = kv->allow + (int64_t)done * r.allow_q_stride;
        r.allow_words = kv->words;
    }
}

// The checks of a key-column request against the rows this launch group scans (read once: IndexView).
int check_key_rows(const EmitRequest& r, const IndexView& iv) {
    if (!r.keys) return RASS_OK;
    if (r.n_keys < iv.rows)
        return fail(RASS_ERR_INVALID, "n_keys (" + std::to_string(r.n_keys) + ") is smaller than the index's rows (" + std::to_string(iv.rows) + ")");
    if (r.allow && r.allow_words < (iv.rows + 31) / 32)
        return fail(RASS_ERR_INVALID, "words_per_bitmap (" + std::to_string(r.allow_words) + ") is smaller than ceil(rows / 32) = " +
                                          std::to_string((iv.rows + 31) / 32));
    return RASS_OK;
}

// ... and its fields of the launch that starts at query q0 of the group.
void key_scan_args(rass::ScanArgs& a, const EmitRequest& r, const IndexView& iv, int q0) {
    if (!r.keys) return;
    a.group_keys = r.keys;
    a.group_key_rows = (int)iv.rows;
    if (r.allow) a.allow = r.allow + (int64_t)q0 * r.allow_q_stride, a.allow_q_stride = r.allow_q_stride;
}

// Where every scan keeps its queries: the head of the engine scratch.
float* emit_queries(const rass_engine* eng) { return range_layout(eng->d_scratch).q_padded; }

// The two halves of the scan of one launch group (<= 32 queries) of an emitting search, the caller's memset of what the scan
// emits into between them and its finishing launch behind them.  Always the exact fp32 scan: the prefilter mode of the index
// is not looked at.  The caller holds eng->mu, has set the device and has checked the arguments.
// emit_begin: the refusals, before the caller grows or zeroes anything, and the queries normalised into the scratch.
int emit_begin(rass_index* idx, const EmitRequest& r, const IndexView& iv) {
    const rass_engine* eng = idx->eng;
    if (iv.rows < 0 || iv.rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (!rass::scan_supported_stride(idx->stride) || idx->stride > kMaxStride) return fail(RASS_ERR_UNSUPPORTED, kStrideMsg);
    if (range_layout(nullptr).total > eng->scratch_bytes) return fail(RASS_ERR_INVALID, "scan workspace too small");
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, emit_queries(eng), idx->stride, r.nq, idx->dim, eng->stream, pad_nq(r.nq)));
    return RASS_OK;
}

// emit_scan: the scan itself (two launches for 17..32 queries on wide rows), `mode(a, q0)` setting the mode's own fields of
// the launch that starts at query q0.  scan_empty: launch over an index of zero rows too (false: skip the scan then).
template <class Mode>
int emit_scan(rass_index* idx, const EmitRequest& r, const IndexView& iv, bool scan_empty, Mode&& mode) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq;
    const int64_t stride = idx->stride;
    float* q_padded = emit_queries(eng);
    const int grid = scan_grid((iv.rows + 31) / 32, 1, eng->n_cus);
    // wide rows: 16 queries per launch, as for the top-k scan (scan_launch)
    const int per_launch = stride > kNarrowStride ? 16 : RASS_MAX_QBATCH;
    for (int q0 = 0; q0 < nq && (scan_empty || iv.rows > 0); q0 += per_launch) {
        rass::ScanArgs a;
        a.corpus = iv.corpus;
        a.row_tag = iv.row_tag;
        a.q_padded = q_padded + (int64_t)q0 * stride;
        a.q_filter = r.q_filter ? r.q_filter + q0 : nullptr;
        a.q_filter_mask = r.q_filter_mask ? r.q_filter_mask + q0 : nullptr;
        a.part_scores = nullptr;
        a.part_ids = nullptr;
        a.row_stride = stride;
        a.id_base = 0;   // what is emitted names rows of the slab: the finishing launch translates them
        a.n_rows = (int)iv.rows;
        a.nq = std::min(per_launch, nq - q0);
        a.k = 1;
        a.xcd_skew = scan_xcd_skew(a.nq, grid, eng->n_cus);
        mode(a, q0);
        const int rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, grid, st)); });
        if (rc != RASS_OK) return rc;
    }
    return RASS_OK;
}

// The checks every entry point here shares; `what` names the search in the message.
int check_exact_f32(const rass_index* idx, const char* what, const int32_t* q_filter, const int32_t* q_filter_mask) {
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, std::string(what) + " needs an fp32 index");
    return RASS_OK;
}

// ... and the two of the grouped search and the aggregation.
int check_groups(int32_t group_mask, int32_t n_groups) {
    if (group_mask <= 0) return fail(RASS_ERR_INVALID, "group_mask must be non-zero and within 0x7fffffff");
    if (n_groups < 1 || n_groups > rass::kGroupMaxGroups) return fail(RASS_ERR_INVALID, "n_groups must be in [1, 1048576]");
    return RASS_OK;
}

// The engine lock and the device, then `group()`: what the three device entry points do once their arguments are checked.
template <class Group>
int device_locked(rass_index* idx, Group&& group) {
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    const int rc = set_device(eng);
    return rc != RASS_OK ? rc : group();
}

// ---- the score-threshold (range) search.  One launch group: normalise -> zero the counters -> the range scan -> range_finish.
struct RangeRequest : EmitRequest {
    const float* min_score = nullptr;   // [nq]
    int max_hits = 0;
    float* out_scores = nullptr;        // [nq][max_hits]
    int64_t* out_ids = nullptr;
    int64_t* total = nullptr;           // [nq]
};

int range_device_group(rass_index* idx, const RangeRequest& r) {
    hipStream_t st = idx->eng->stream;
    // the tags are read only where the call filters or a row is deleted
    const IndexView iv = index_view(idx, /*filtered=*/r.q_filter != nullptr, r.id_base);
    if (int rc = emit_begin(idx, r, iv)) return rc;
    const RangeView L = range_layout(idx->eng->d_scratch);
    HIP_TRY(hipMemsetAsync(L.count, 0, (size_t)RASS_MAX_QBATCH * rass::kRangeCountStride * sizeof(unsigned), st));
    // scan_empty: the range scan has always been launched over an empty index as well (one launch group in the kernel timing)
    const int rc = emit_scan(idx, r, iv, /*scan_empty=*/true, [&](rass::ScanArgs& a, int q0) {
        a.range_thr = r.min_score + q0;
        a.range_count = L.count + q0 * rass::kRangeCountStride;
        a.range_hits = L.hits + (int64_t)q0 * r.max_hits;
        a.range_cap = r.max_hits;
    });
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_range_finish(L.count, L.hits, r.nq, r.max_hits, iv.id_base, iv.id_map, r.out_scores, r.out_ids, r.total, st));
    return RASS_OK;
}

int check_range(const rass_index* idx, int max_hits, const int32_t* q_filter, const int32_t* q_filter_mask) {
    if (max_hits < 1 || max_hits > RASS_MAX_K_MULTIPASS) return fail(RASS_ERR_INVALID, "max_hits must be in [1, RASS_MAX_K_MULTIPASS]");
    return check_exact_f32(idx, "range search", q_filter, q_filter_mask);
}

// One attempt of the host range search.  Phase 1: group by group through a pinned slot (host_groups).  Phase 2, with the slot
// released: the queries whose total exceeds max_hits get the best max_hits matching rows — more than max_hits rows reach the
// threshold, so those are the plain top max_hits under the query's filter — from the multipass top-k path itself, pinned to
// the exact scan.
int search_range_once(rass_index* idx, const float* queries, int nq, const float* min_score, int max_hits, const int32_t* q_filter,
                      const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids, int64_t* out_total) {
    rass_engine* eng = idx->eng;
    int rc = host_groups(
        idx, queries, nq, q_filter, q_filter_mask, range_io_layout(nullptr).bytes,
        [&](HostSlot* sl, int done, int b) {
            memcpy(range_io_layout(static_cast<unsigned char*>(sl->h_io)).thr, min_score + done, (size_t)b * sizeof(float));
        },
        [&](HostSlot* sl, int, int b) -> int {
            hipStream_t st = eng->stream;
            const RangeIoView H = range_io_layout(static_cast<unsigned char*>(sl->h_io)), D = range_io_layout(eng->d_io);
            const size_t cells = (size_t)b * max_hits;
            HIP_TRY(hipMemcpyAsync(D.thr, H.thr, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            RangeRequest r;
            r.queries = eng->d_qraw, r.nq = b, r.min_score = D.thr, r.max_hits = max_hits;
            r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = D.out_scores, r.out_ids = D.out_ids, r.total = D.total;
            if (int grc = range_device_group(idx, r)) return grc;
            HIP_TRY(hipMemcpyAsync(H.total, D.total, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_scores, D.out_scores, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_ids, D.out_ids, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            const RangeIoView H = range_io_layout(static_cast<unsigned char*>(sl->h_io));
            const size_t cells = (size_t)b * max_hits;
            memcpy(out_total + done, H.total, (size_t)b * sizeof(int64_t));
            memcpy(out_scores + (int64_t)done * max_hits, H.out_scores, cells * sizeof(float));
            memcpy(out_ids + (int64_t)done * max_hits, H.out_ids, cells * sizeof(int64_t));
            return RASS_OK;
        });
    if (rc != RASS_OK) return rc;
    std::vector<int> over;
    for (int q = 0; q < nq; ++q)
        if (out_total[q] > max_hits) over.push_back(q);
    if (over.empty()) return RASS_OK;
    const int no = (int)over.size(), dim = idx->dim;
    std::vector<float> oq((size_t)no * dim), os((size_t)no * max_hits);
    std::vector<int32_t> of(q_filter ? no : 0), om(q_filter_mask ? no : 0);
    std::vector<int64_t> oi((size_t)no * max_hits);
    for (int j = 0; j < no; ++j) {
        memcpy(oq.data() + (size_t)j * dim, queries + (int64_t)over[j] * dim, (size_t)dim * sizeof(float));
        if (q_filter) of[j] = q_filter[over[j]];
        if (q_filter_mask) om[j] = q_filter_mask[over[j]];
    }
    rc = search_ex_once(idx, oq.data(), no, max_hits, q_filter ? of.data() : nullptr, q_filter_mask ? om.data() : nullptr, os.data(),
                        oi.data(), /*exact=*/true);
    if (rc != RASS_OK) return rc;
    for (int j = 0; j < no; ++j) {
        memcpy(out_scores + (int64_t)over[j] * max_hits, os.data() + (size_t)j * max_hits, (size_t)max_hits * sizeof(float));
        memcpy(out_ids + (int64_t)over[j] * max_hits, oi.data() + (size_t)j * max_hits, (size_t)max_hits * sizeof(int64_t));
    }
    return RASS_OK;
}

// ---- the grouped (collapsed) search.  One launch group: normalise -> zero the status word and the table -> the group-max scan ->
// group_select.
struct GroupRequest : EmitRequest {
    int k = 0;
    int32_t group_mask = 0;
    int32_t n_groups = 0;
    float* out_scores = nullptr;        // [nq][k]
    int64_t* out_ids = nullptr;
    int32_t* out_groups = nullptr;
    int64_t* total = nullptr;           // [nq]
    int32_t* status = nullptr;          // [1]
};

}  // namespace

// The table block at least `need` bytes (api_internal.h; api_grouptop.hip grows it too).  The new block is allocated BEFORE the
// old one is let go: a failure leaves the engine as it was.  Growth waits for the stream first: an earlier call on it may still use the old block.
int grow_group_table(rass_engine* eng, size_t need, hipStream_t st, const char* who) {
    if (eng->group_bytes >= need) return RASS_OK;
    unsigned char* block = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&block), need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RASS_ERR_OOM, std::string(who) + ": hipMalloc of the group table (" + std::to_string(need) + " bytes) failed");
    }
    const int rc = HIP_RC(hipStreamSynchronize(st));
    if (rc != RASS_OK) {
        (void)hipFree(block);
        return rc;
    }
    if (eng->d_group) (void)hipFree(eng->d_group);
    eng->d_group = block;
    eng->group_bytes = need;
    return RASS_OK;
}

namespace {

int group_device_group(rass_index* idx, const GroupRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const IndexView iv = index_view(idx, /*filtered=*/true, r.id_base);   // the group key is in the tag: always read them
    if (int rc = check_key_rows(r, iv)) return rc;
    if (int rc = emit_begin(idx, r, iv)) return rc;
    if (int rc = grow_group_table(eng, group_layout(nullptr, r.nq, r.n_groups).total, st, "grouped search")) return rc;
    const GroupView G = group_layout(eng->d_group, r.nq, r.n_groups);
    HIP_TRY(hipMemsetAsync(G.status, 0, G.total, st));
    // an empty index is not scanned: the zeroed table is the answer
    const int rc = emit_scan(idx, r, iv, /*scan_empty=*/false, [&](rass::ScanArgs& a, int q0) {
        a.group_table = G.table + (int64_t)q0 * r.n_groups;
        a.group_status = G.status;
        a.group_mask = r.group_mask;
        a.group_shift = __builtin_ctz((unsigned)r.group_mask);
        a.group_n = r.n_groups;
        key_scan_args(a, r, iv, q0);
    });
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_group_select(G.table, r.nq, r.n_groups, r.k, iv.id_base, iv.id_map, r.out_scores, r.out_ids, r.out_groups,
                                      r.total, G.status, r.status, st));
    return RASS_OK;
}

int check_grouped(const rass_index* idx, int k, int32_t group_mask, int32_t n_groups, const int32_t* q_filter,
                  const int32_t* q_filter_mask) {
    if (k < 1 || k > RASS_MAX_K_MULTIPASS) return fail(RASS_ERR_INVALID, "k must be in [1, RASS_MAX_K_MULTIPASS]");
    if (int rc = check_groups(group_mask, n_groups)) return rc;
    return check_exact_f32(idx, "grouped search", q_filter, q_filter_mask);
}

// One attempt of the host grouped search.  A group whose scan met a group key >= n_groups ends the call.
int search_grouped_once(rass_index* idx, const float* queries, int nq, int k, int32_t group_mask, int32_t n_groups,
                        const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids, int32_t* out_groups,
                        int64_t* out_total, const KeyArgs* kv = nullptr) {
    rass_engine* eng = idx->eng;
    return host_groups(
        idx, queries, nq, q_filter, q_filter_mask, group_io_layout(nullptr).bytes, no_fill,
        [&](HostSlot* sl, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const GroupIoView H = group_io_layout(static_cast<unsigned char*>(sl->h_io)), D = group_io_layout(eng->d_io);
            const size_t cells = (size_t)b * k;
            GroupRequest r;
            key_request(r, kv, done);
            r.queries = eng->d_qraw, r.nq = b, r.k = k, r.group_mask = group_mask, r.n_groups = n_groups;
            r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = D.out_scores, r.out_ids = D.out_ids, r.out_groups = D.out_groups, r.total = D.total, r.status = D.status;
            if (int grc = group_device_group(idx, r)) return grc;
            HIP_TRY(hipMemcpyAsync(H.total, D.total, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.status, D.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_scores, D.out_scores, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_ids, D.out_ids, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_groups, D.out_groups, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            const GroupIoView H = group_io_layout(static_cast<unsigned char*>(sl->h_io));
            const size_t cells = (size_t)b * k;
            if (*H.status != 0)
                return fail(RASS_ERR_INVALID, "grouped search: a matching row's group key is >= n_groups (" + std::to_string(n_groups) + ")");
            memcpy(out_total + done, H.total, (size_t)b * sizeof(int64_t));
            memcpy(out_scores + (int64_t)done * k, H.out_scores, cells * sizeof(float));
            memcpy(out_ids + (int64_t)done * k, H.out_ids, cells * sizeof(int64_t));
            memcpy(out_groups + (int64_t)done * k, H.out_groups, cells * sizeof(int32_t));
            return RASS_OK;
        });
}

// ---- the terms aggregation.  One launch group: normalise -> ONE memset over the status word, the best-row table and the
// counters -> the group-count scan -> the select over the counters.
struct AggRequest : EmitRequest {
    const float* min_score = nullptr;   // [nq]
    int size = 0;
    int32_t group_mask = 0;
    int32_t n_groups = 0;
    int32_t* out_groups = nullptr;      // [nq][size]
    int64_t* out_counts = nullptr;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    int64_t* n_buckets = nullptr;       // [nq]
    int64_t* total_hits = nullptr;      // [nq]
    int32_t* status = nullptr;          // [1]
};

int agg_device_group(rass_index* idx, const AggRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const IndexView iv = index_view(idx, /*filtered=*/true, r.id_base);   // the group key is in the tag: always read them
    if (int rc = check_key_rows(r, iv)) return rc;
    if (int rc = emit_begin(idx, r, iv)) return rc;
    if (int rc = grow_group_table(eng, agg_layout(nullptr, r.nq, r.n_groups).total, st, "aggregation")) return rc;
    const AggView G = agg_layout(eng->d_group, r.nq, r.n_groups);
    HIP_TRY(hipMemsetAsync(G.status, 0, G.total, st));
    // an empty index is not scanned: the zeroed tables are the answer
    const int rc = emit_scan(idx, r, iv, /*scan_empty=*/false, [&](rass::ScanArgs& a, int q0) {
        a.range_thr = r.min_score + q0;
        a.group_table = G.best + (int64_t)q0 * r.n_groups;
        a.count_table = G.count + (int64_t)q0 * r.n_groups;
        a.group_status = G.status;
        a.group_mask = r.group_mask;
        a.group_shift = __builtin_ctz((unsigned)r.group_mask);
        a.group_n = r.n_groups;
        key_scan_args(a, r, iv, q0);
    });
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_group_count_select(G.count, G.best, r.nq, r.n_groups, r.size, iv.id_base, iv.id_map, r.out_groups, r.out_counts,
                                            r.out_scores, r.out_ids, r.n_buckets, r.total_hits, G.status, r.status, st));
    return RASS_OK;
}

int check_aggregate(const rass_index* idx, int size, int32_t group_mask, int32_t n_groups, const int32_t* q_filter,
                    const int32_t* q_filter_mask) {
    if (size < 1 || size > rass::kGroupMaxK) return fail(RASS_ERR_INVALID, "size must be in [1, RASS_MAX_K_MULTIPASS]");
    if (int rc = check_groups(group_mask, n_groups)) return rc;
    return check_exact_f32(idx, "aggregation", q_filter, q_filter_mask);
}

// One attempt of the host aggregation.  A group whose scan met a hit with a group key >= n_groups ends the call.
int aggregate_once(rass_index* idx, const float* queries, int nq, const float* min_score, int size, int32_t group_mask,
                   int32_t n_groups, const int32_t* q_filter, const int32_t* q_filter_mask, int32_t* out_groups, int64_t* out_counts,
                   float* out_scores, int64_t* out_ids, int64_t* out_n_buckets, int64_t* out_total_hits, const KeyArgs* kv = nullptr) {
    rass_engine* eng = idx->eng;
    return host_groups(
        idx, queries, nq, q_filter, q_filter_mask, agg_io_layout(nullptr).bytes,
        [&](HostSlot* sl, int done, int b) {
            memcpy(agg_io_layout(static_cast<unsigned char*>(sl->h_io)).thr, min_score + done, (size_t)b * sizeof(float));
        },
        [&](HostSlot* sl, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const AggIoView H = agg_io_layout(static_cast<unsigned char*>(sl->h_io)), D = agg_io_layout(eng->d_io);
            const size_t cells = (size_t)b * size;
            HIP_TRY(hipMemcpyAsync(D.thr, H.thr, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            AggRequest r;
            key_request(r, kv, done);
            r.queries = eng->d_qraw, r.nq = b, r.min_score = D.thr, r.size = size, r.group_mask = group_mask, r.n_groups = n_groups;
            r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            r.out_groups = D.out_groups, r.out_counts = D.out_counts, r.out_scores = D.out_scores, r.out_ids = D.out_ids;
            r.n_buckets = D.n_buckets, r.total_hits = D.total_hits, r.status = D.status;
            if (int grc = agg_device_group(idx, r)) return grc;
            HIP_TRY(hipMemcpyAsync(H.n_buckets, D.n_buckets, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.total_hits, D.total_hits, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.status, D.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_groups, D.out_groups, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_counts, D.out_counts, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_scores, D.out_scores, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_ids, D.out_ids, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            const AggIoView H = agg_io_layout(static_cast<unsigned char*>(sl->h_io));
            const size_t cells = (size_t)b * size;
            if (*H.status != 0)
                return fail(RASS_ERR_INVALID, "aggregation: a hit's group key is >= n_groups (" + std::to_string(n_groups) + ")");
            memcpy(out_n_buckets + done, H.n_buckets, (size_t)b * sizeof(int64_t));
            memcpy(out_total_hits + done, H.total_hits, (size_t)b * sizeof(int64_t));
            memcpy(out_groups + (int64_t)done * size, H.out_groups, cells * sizeof(int32_t));
            memcpy(out_counts + (int64_t)done * size, H.out_counts, cells * sizeof(int64_t));
            memcpy(out_scores + (int64_t)done * size, H.out_scores, cells * sizeof(float));
            memcpy(out_ids + (int64_t)done * size, H.out_ids, cells * sizeof(int64_t));
            return RASS_OK;
        });
}

// The arguments every key-column entry point adds.
int check_keys(const rass_index* idx, const KeyArgs& kv, int nq) {
    if (!kv.keys) return fail(RASS_ERR_INVALID, "d_keys is NULL");
    if (kv.n_keys < 0) return fail(RASS_ERR_INVALID, "n_keys is negative");
    if (!kv.allow) return RASS_OK;
    if (kv.n_bitmaps != 1 && kv.n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
    if (kv.words < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "a bitmap with a key column needs dim <= 1024");
    return RASS_OK;
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_search_range_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int max_hits,
                                   const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base,
                                   float* d_out_scores, int64_t* d_out_ids, int64_t* d_total) {
    if (!idx || !d_queries || !d_min_score || !d_out_scores || !d_out_ids || !d_total) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_range(idx, max_hits, d_q_filter, d_q_filter_mask)) return rc;
    RangeRequest r;
    r.queries = d_queries, r.nq = nq, r.min_score = d_min_score, r.max_hits = max_hits;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_scores = d_out_scores, r.out_ids = d_out_ids, r.total = d_total;
    return device_locked(idx, [&] { return range_device_group(idx, r); });
}

int rass_index_search_range(rass_index_t* idx, const float* queries, int nq, const float* min_score, int max_hits,
                            const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids,
                            int64_t* out_total) {
    if (!idx || !out_scores || !out_ids || !out_total) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && (!queries || !min_score))) return fail(RASS_ERR_INVALID, "bad queries / min_score / nq");
    if (int rc = check_range(idx, max_hits, q_filter, q_filter_mask)) return rc;
    for (int q = 0; q < nq; ++q)
        if (min_score[q] != min_score[q]) return fail(RASS_ERR_INVALID, "min_score is NaN");
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return search_range_once(idx, queries, nq, min_score, max_hits, q_filter, q_filter_mask, out_scores, out_ids, out_total);
    });
}

int rass_index_search_grouped_device(rass_index_t* idx, const float* d_queries, int nq, int k, int32_t group_mask, int32_t n_groups,
                                     const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base,
                                     float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_groups, int64_t* d_group_total,
                                     int32_t* d_status) {
    if (!idx || !d_queries || !d_out_scores || !d_out_ids || !d_out_groups || !d_group_total || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_grouped(idx, k, group_mask, n_groups, d_q_filter, d_q_filter_mask)) return rc;
    GroupRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.group_mask = group_mask, r.n_groups = n_groups;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_scores = d_out_scores, r.out_ids = d_out_ids, r.out_groups = d_out_groups, r.total = d_group_total, r.status = d_status;
    return device_locked(idx, [&] { return group_device_group(idx, r); });
}

int rass_index_search_grouped(rass_index_t* idx, const float* queries, int nq, int k, int32_t group_mask, int32_t n_groups,
                              const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids,
                              int32_t* out_groups, int64_t* out_group_total) {
    if (!idx || !out_scores || !out_ids || !out_groups || !out_group_total) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_grouped(idx, k, group_mask, n_groups, q_filter, q_filter_mask)) return rc;
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return search_grouped_once(idx, queries, nq, k, group_mask, n_groups, q_filter, q_filter_mask, out_scores, out_ids, out_groups,
                                   out_group_total);
    });
}

int rass_index_aggregate_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                int32_t group_mask, int32_t n_groups, const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                int64_t id_base, int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores,
                                int64_t* d_out_ids, int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status) {
    if (!idx || !d_queries || !d_min_score || !d_out_groups || !d_out_counts || !d_out_scores || !d_out_ids || !d_n_buckets ||
        !d_total_hits || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_aggregate(idx, size, group_mask, n_groups, d_q_filter, d_q_filter_mask)) return rc;
    AggRequest r;
    r.queries = d_queries, r.nq = nq, r.min_score = d_min_score, r.size = size, r.group_mask = group_mask, r.n_groups = n_groups;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_groups = d_out_groups, r.out_counts = d_out_counts, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    r.n_buckets = d_n_buckets, r.total_hits = d_total_hits, r.status = d_status;
    return device_locked(idx, [&] { return agg_device_group(idx, r); });
}

int rass_index_aggregate(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size, int32_t group_mask,
                         int32_t n_groups, const int32_t* q_filter, const int32_t* q_filter_mask, int32_t* out_groups,
                         int64_t* out_counts, float* out_scores, int64_t* out_ids, int64_t* out_n_buckets, int64_t* out_total_hits) {
    if (!idx || !out_groups || !out_counts || !out_scores || !out_ids || !out_n_buckets || !out_total_hits)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && (!queries || !min_score))) return fail(RASS_ERR_INVALID, "bad queries / min_score / nq");
    if (int rc = check_aggregate(idx, size, group_mask, n_groups, q_filter, q_filter_mask)) return rc;
    for (int q = 0; q < nq; ++q)
        if (min_score[q] != min_score[q]) return fail(RASS_ERR_INVALID, "min_score is NaN");
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return aggregate_once(idx, queries, nq, min_score, size, group_mask, n_groups, q_filter, q_filter_mask, out_groups, out_counts,
                              out_scores, out_ids, out_n_buckets, out_total_hits);
    });
}

int rass_index_search_grouped_keys_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_keys,
                                          int64_t n_keys, int32_t n_groups, const uint32_t* d_allow, int n_bitmaps,
                                          int64_t words_per_bitmap, const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                          int64_t id_base, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_groups,
                                          int64_t* d_group_total, int32_t* d_status) {
    if (!idx || !d_queries || !d_out_scores || !d_out_ids || !d_out_groups || !d_group_total || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_grouped(idx, k, kWholeKey, n_groups, d_q_filter, d_q_filter_mask)) return rc;
    const KeyArgs kv{d_keys, n_keys, d_allow, n_bitmaps, words_per_bitmap};
    if (int rc = check_keys(idx, kv, nq)) return rc;
    GroupRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.group_mask = kWholeKey, r.n_groups = n_groups;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_scores = d_out_scores, r.out_ids = d_out_ids, r.out_groups = d_out_groups, r.total = d_group_total, r.status = d_status;
    key_request(r, &kv, 0);
    return device_locked(idx, [&] { return group_device_group(idx, r); });
}

int rass_index_search_grouped_keys(rass_index_t* idx, const float* queries, int nq, int k, const int32_t* d_keys, int64_t n_keys,
                                   int32_t n_groups, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                   const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids,
                                   int32_t* out_groups, int64_t* out_group_total) {
    if (!idx || !out_scores || !out_ids || !out_groups || !out_group_total) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_grouped(idx, k, kWholeKey, n_groups, q_filter, q_filter_mask)) return rc;
    const KeyArgs kv{d_keys, n_keys, d_allow, n_bitmaps, words_per_bitmap};
    if (int rc = check_keys(idx, kv, nq)) return rc;
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return search_grouped_once(idx, queries, nq, k, kWholeKey, n_groups, q_filter, q_filter_mask, out_scores, out_ids, out_groups,
                                   out_group_total, &kv);
    });
}

int rass_index_aggregate_keys_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                     const int32_t* d_keys, int64_t n_keys, int32_t n_groups, const uint32_t* d_allow, int n_bitmaps,
                                     int64_t words_per_bitmap, const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                     int64_t id_base, int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores,
                                     int64_t* d_out_ids, int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status) {
    if (!idx || !d_queries || !d_min_score || !d_out_groups || !d_out_counts || !d_out_scores || !d_out_ids || !d_n_buckets ||
        !d_total_hits || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_aggregate(idx, size, kWholeKey, n_groups, d_q_filter, d_q_filter_mask)) return rc;
    const KeyArgs kv{d_keys, n_keys, d_allow, n_bitmaps, words_per_bitmap};
    if (int rc = check_keys(idx, kv, nq)) return rc;
    AggRequest r;
    r.queries = d_queries, r.nq = nq, r.min_score = d_min_score, r.size = size, r.group_mask = kWholeKey, r.n_groups = n_groups;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_groups = d_out_groups, r.out_counts = d_out_counts, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    r.n_buckets = d_n_buckets, r.total_hits = d_total_hits, r.status = d_status;
    key_request(r, &kv, 0);
    return device_locked(idx, [&] { return agg_device_group(idx, r); });
}

int rass_index_aggregate_keys(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                              const int32_t* d_keys, int64_t n_keys, int32_t n_groups, const uint32_t* d_allow, int n_bitmaps,
                              int64_t words_per_bitmap, const int32_t* q_filter, const int32_t* q_filter_mask, int32_t* out_groups,
                              int64_t* out_counts, float* out_scores, int64_t* out_ids, int64_t* out_n_buckets,
                              int64_t* out_total_hits) {
    if (!idx || !out_groups || !out_counts || !out_scores || !out_ids || !out_n_buckets || !out_total_hits)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && (!queries || !min_score))) return fail(RASS_ERR_INVALID, "bad queries / min_score / nq");
    if (int rc = check_aggregate(idx, size, kWholeKey, n_groups, q_filter, q_filter_mask)) return rc;
    const KeyArgs kv{d_keys, n_keys, d_allow, n_bitmaps, words_per_bitmap};
    if (int rc = check_keys(idx, kv, nq)) return rc;
    for (int q = 0; q < nq; ++q)
        if (min_score[q] != min_score[q]) return fail(RASS_ERR_INVALID, "min_score is NaN");
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return aggregate_once(idx, queries, nq, min_score, size, kWholeKey, n_groups, q_filter, q_filter_mask, out_groups, out_counts,
                              out_scores, out_ids, out_n_buckets, out_total_hits, &kv);
    });
}

}  // extern "C"
