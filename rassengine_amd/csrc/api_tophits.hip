// api_tophits.hip — the C ABI of include/rass_engine.h: the terms aggregation over a key column with a top_hits sub-aggregation,
// rass_index_aggregate_hits_keys(_device): rass_index_aggregate_keys' buckets, each with its top_hits best hits, ordered by
// doc_count or by the best hit.  Host-side C++ only: the kernels are scan_tophits.hip (the one-pass scan into a level-major
// table and a counter plane) and group_topk.hip (either select, unchanged, then group_hits_finish_kernel over the listed
// buckets and, under the score order, the gather of their counters).  The table lives in the engine-owned block of the grouped
// search (eng->d_group).  The objects and the threading rules: api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// One launch group (<= 32 queries).  Everything is a device pointer.
struct TopHitsRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    const float* min_score = nullptr;   // [nq]
    const uint32_t* allow = nullptr;    // this launch group's bitmap(s); allow_q_stride 0: one shared by all of them
    int64_t allow_q_stride = 0, allow_words = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    int32_t* out_groups = nullptr;      // [nq][size]
    int64_t* out_counts = nullptr;
    float* out_scores = nullptr;        // [nq][size][top_hits]
    int64_t* out_ids = nullptr;
    int64_t* n_buckets = nullptr;       // [nq]
    int64_t* total_hits = nullptr;      // [nq]
    int32_t* status = nullptr;          // [1]
};

// What the caller passed, whole.
struct TopHitsCall {
    int size;
    const int32_t* keys;
    int64_t n_keys;
    int32_t n_groups;
    int top_hits, order_by;
    const uint32_t* allow;
    int n_bitmaps;
    int64_t words;
    const int32_t* q_filter;
    const int32_t* q_filter_mask;
};

// ... and a launch group's part of it.
void tophits_request(TopHitsRequest& r, const TopHitsCall& a, int done) {
    if (a.allow) {
        r.allow_q_stride = a.n_bitmaps == 1 ? 0 : a.words;
        r.allow = a.allow + (int64_t)done * r.allow_q_stride;
        r.allow_words = a.words;
    }
}

// The argument checks the two entry points share (everything that does not need the row count).
int check_tophits(const rass_index* idx, const TopHitsCall& a, int nq) {
    if (a.size < 1 || a.size > rass::kGroupMaxK) return fail(RASS_ERR_INVALID, "size must be in [1, RASS_MAX_K_MULTIPASS]");
    if (a.n_groups < 1 || a.n_groups > rass::kGroupMaxGroups) return fail(RASS_ERR_INVALID, "n_groups must be in [1, 1048576]");
    if (a.top_hits < 1 || a.top_hits > RASS_MAX_GROUP_SIZE) return fail(RASS_ERR_INVALID, "top_hits must be in [1, RASS_MAX_GROUP_SIZE]");
    if ((int64_t)a.n_groups * a.top_hits > rass::kGroupMaxGroups)
        return fail(RASS_ERR_INVALID, "n_groups * top_hits must not exceed 1048576");
    if (a.order_by != RASS_AGG_BY_COUNT && a.order_by != RASS_AGG_BY_SCORE)
        return fail(RASS_ERR_INVALID, "order_by must be RASS_AGG_BY_COUNT or RASS_AGG_BY_SCORE");
    if (a.q_filter_mask && !a.q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (!a.keys) return fail(RASS_ERR_INVALID, "d_keys is NULL");
    if (a.n_keys < 0) return fail(RASS_ERR_INVALID, "n_keys is negative");
    if (a.allow) {
        if (a.n_bitmaps != 1 && a.n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
        if (a.words < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    }
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "top-hits aggregation needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "top-hits aggregation needs dim <= 1024 (no wide-row form)");
    return RASS_OK;
}

// The table block (eng->d_group, one launch group): the status word, top_hits level-major planes of [nq][n_groups] 64-bit
// slots (plane 0: the best hit), one plane of counters.  All adjacent: one memset zeroes everything, and the zeroed table is
// the empty one.  At most 32 x 2^20 x 8 bytes of levels and 128 MiB of counters.
struct TopHitsView {
    unsigned* status;              // [2] on a 256-byte line: the scan's word, and a spare one for the select's copy of it
    unsigned long long* table;     // [top_hits][nq][n_groups]
    unsigned* count;               // [nq][n_groups]
    size_t total;
};
TopHitsView tophits_layout(unsigned char* base, int nq, int n_groups, int top_hits) {
    Carver c{base};
    TopHitsView L;
    const size_t slots = (size_t)nq * n_groups;
    L.status = c.take<unsigned>(2 * sizeof(unsigned));
    L.table = c.take<unsigned long long>(slots * top_hits * sizeof(unsigned long long));
    L.count = c.take<unsigned>(slots * sizeof(unsigned));
    L.total = c.off;
    return L;
}

// normalise -> ONE memset over the status word, every level and the counters -> the top-hits scan -> the select (by the
// counters, or over plane 0) -> the finish over the listed buckets (-> the counters' gather).  Always the exact fp32 scan: the
// prefilter mode of the index is not looked at.  The caller holds eng->mu and has set the device.
int tophits_device_group(rass_index* idx, const TopHitsRequest& r, const TopHitsCall& a) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const IndexView iv = index_view(idx, /*filtered=*/true, r.id_base);   // tombstones and filters: always read the tags
    if (a.n_keys < iv.rows)
        return fail(RASS_ERR_INVALID, "n_keys (" + std::to_string(a.n_keys) + ") is smaller than the index's rows (" + std::to_string(iv.rows) + ")");
    if (r.allow)
        if (int rc = check_words(iv.rows, r.allow_words)) return rc;
    if (iv.rows < 0 || iv.rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (range_layout(nullptr).total > eng->scratch_bytes) return fail(RASS_ERR_INVALID, "scan workspace too small");
    if (int rc = grow_group_table(eng, tophits_layout(nullptr, r.nq, a.n_groups, a.top_hits).total, st, "top-hits aggregation")) return rc;
    float* q_padded = range_layout(eng->d_scratch).q_padded;   // where every scan keeps its queries
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, q_padded, idx->stride, r.nq, idx->dim, st, pad_nq(r.nq)));
    const TopHitsView G = tophits_layout(eng->d_group, r.nq, a.n_groups, a.top_hits);
    HIP_TRY(hipMemsetAsync(G.status, 0, G.total, st));
    if (iv.rows > 0) {   // an empty index is not scanned: the zeroed table is the answer
        const int grid = scan_grid((iv.rows + 31) / 32, 1, eng->n_cus);
        rass::TopHitsArgs s;
        s.scan.corpus = iv.corpus;
        s.scan.row_tag = iv.row_tag;
        s.scan.q_padded = q_padded;
        s.scan.q_filter = r.q_filter;
        s.scan.q_filter_mask = r.q_filter_mask;
        s.scan.part_scores = nullptr;
        s.scan.part_ids = nullptr;
        s.scan.row_stride = idx->stride;
        s.scan.id_base = 0;   // the keys name rows of the slab: the finishing launches translate them
        s.scan.n_rows = (int)iv.rows;
        s.scan.nq = r.nq;
        s.scan.k = 1;
        s.scan.range_thr = r.min_score;
        s.scan.group_table = G.table;
        s.scan.group_status = G.status;
        s.scan.group_n = a.n_groups;
        s.scan.group_keys = a.keys;
        s.scan.group_key_rows = (int)iv.rows;
        s.scan.allow = r.allow;
        s.scan.allow_q_stride = r.allow_q_stride;
        s.count = G.count;
        s.level_stride = (int64_t)r.nq * a.n_groups;
        s.top_hits = a.top_hits;
        const int rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_tophits_f32(s, grid, st)); });
        if (rc != RASS_OK) return rc;
    }
    // The select's own [nq][size] scores and ids (each bucket's best hit) land in the head of the three-dimensional outputs,
    // which the finish then overwrites whole without reading them; its copy of the status word goes to the spare word.
    int32_t* spare = reinterpret_cast<int32_t*>(G.status + 1);
    if (a.order_by == RASS_AGG_BY_COUNT)
        HIP_TRY(rass::launch_group_count_select(G.count, G.table, r.nq, a.n_groups, a.size, iv.id_base, iv.id_map, r.out_groups,
                                                r.out_counts, r.out_scores, r.out_ids, r.n_buckets, r.total_hits, G.status, spare, st));
    else   // plane 0 holds hits only: its non-zero slots are the buckets
        HIP_TRY(rass::launch_group_select(G.table, r.nq, a.n_groups, a.size, iv.id_base, iv.id_map, r.out_scores, r.out_ids, r.out_groups,
                                          r.n_buckets, G.status, spare, st));
    HIP_TRY(rass::launch_group_hits_finish(G.table, r.nq, a.n_groups, a.size, a.top_hits, iv.id_base, iv.id_map, r.out_groups,
                                           r.out_scores, r.out_ids, nullptr, nullptr, G.status, r.status, /*accumulate=*/false, st));
    if (a.order_by != RASS_AGG_BY_COUNT)
        HIP_TRY(rass::launch_group_counts_gather(r.out_groups, G.count, r.nq, a.n_groups, a.size, r.out_counts, r.total_hits, st));
    return RASS_OK;
}

// The device staging of the host variant's lists (eng->d_allow_io), sized by the call.
struct TopHitsIoView {
    float* out_scores;      // [32][size][top_hits]
    int64_t* out_ids;
    size_t bytes;
};
TopHitsIoView tophits_io_layout(unsigned char* base, int size, int top_hits) {
    Carver c{base};
    TopHitsIoView L;
    const size_t cells = (size_t)RASS_MAX_QBATCH * size * top_hits;
    L.out_scores = c.take<float>(cells * sizeof(float));
    L.out_ids = c.take<int64_t>(cells * sizeof(int64_t));
    L.bytes = c.off;
    return L;
}

// What the host variant writes.
struct TopHitsOut {
    int32_t* groups;
    int64_t* counts;
    float* scores;
    int64_t* ids;
    int64_t* n_buckets;
    int64_t* total_hits;
};

// One attempt of the host call.  Thresholds, per-query figures, status, groups and counts go through the aggregation's pinned
// staging (AggIoView); the lists through the engine's own staging block, straight to the caller's arrays, as the group-hits
// search sends its own.  A group whose scan met a hit with a key >= n_groups ends the call.
int tophits_once(rass_index* idx, const float* queries, int nq, const float* min_score, const TopHitsCall& a, const TopHitsOut& o) {
    rass_engine* eng = idx->eng;
    const int size = a.size, th = a.top_hits;
    return host_groups(
        idx, queries, nq, a.q_filter, a.q_filter_mask, agg_io_layout(nullptr).bytes,
        [&](HostSlot* sl, int done, int b) {
            memcpy(agg_io_layout(static_cast<unsigned char*>(sl->h_io)).thr, min_score + done, (size_t)b * sizeof(float));
        },
        [&](HostSlot* sl, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const AggIoView H = agg_io_layout(static_cast<unsigned char*>(sl->h_io)), D = agg_io_layout(eng->d_io);
            if (int rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, tophits_io_layout(nullptr, size, th).bytes, st)) return rc;
            const TopHitsIoView L = tophits_io_layout(eng->d_allow_io, size, th);
            const size_t cells = (size_t)b * size;
            HIP_TRY(hipMemcpyAsync(D.thr, H.thr, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            TopHitsRequest r;
            tophits_request(r, a, done);
            r.queries = eng->d_qraw, r.nq = b, r.min_score = D.thr;
            r.q_filter = a.q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = a.q_filter_mask ? eng->d_qmask : nullptr;
            r.out_groups = D.out_groups, r.out_counts = D.out_counts, r.out_scores = L.out_scores, r.out_ids = L.out_ids;
            r.n_buckets = D.n_buckets, r.total_hits = D.total_hits, r.status = D.status;
            if (int grc = tophits_device_group(idx, r, a)) return grc;
            HIP_TRY(hipMemcpyAsync(H.n_buckets, D.n_buckets, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.total_hits, D.total_hits, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.status, D.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_groups, D.out_groups, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_counts, D.out_counts, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(o.scores + (int64_t)done * size * th, L.out_scores, cells * th * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(o.ids + (int64_t)done * size * th, L.out_ids, cells * th * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            const AggIoView H = agg_io_layout(static_cast<unsigned char*>(sl->h_io));
            const size_t cells = (size_t)b * size;
            if (*H.status != 0)
                return fail(RASS_ERR_INVALID, "top-hits aggregation: a hit's group key is >= n_groups (" + std::to_string(a.n_groups) + ")");
            memcpy(o.n_buckets + done, H.n_buckets, (size_t)b * sizeof(int64_t));
            memcpy(o.total_hits + done, H.total_hits, (size_t)b * sizeof(int64_t));
            memcpy(o.groups + (int64_t)done * size, H.out_groups, cells * sizeof(int32_t));
            memcpy(o.counts + (int64_t)done * size, H.out_counts, cells * sizeof(int64_t));
            return RASS_OK;
        });
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_aggregate_hits_keys_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                          const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int top_hits, int order_by,
                                          const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                          const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base,
                                          int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores, int64_t* d_out_ids,
                                          int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status) {
    if (!idx || !d_queries || !d_min_score || !d_out_groups || !d_out_counts || !d_out_scores || !d_out_ids || !d_n_buckets ||
        !d_total_hits || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    const TopHitsCall a{size, d_keys, n_keys, n_groups, top_hits, order_by, d_allow, n_bitmaps, words_per_bitmap, d_q_filter,
                        d_q_filter_mask};
    if (int rc = check_tophits(idx, a, nq)) return rc;
    TopHitsRequest r;
    tophits_request(r, a, 0);
    r.queries = d_queries, r.nq = nq, r.min_score = d_min_score;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_groups = d_out_groups, r.out_counts = d_out_counts, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    r.n_buckets = d_n_buckets, r.total_hits = d_total_hits, r.status = d_status;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    const int rc = set_device(eng);
    return rc != RASS_OK ? rc : tophits_device_group(idx, r, a);
}

int rass_index_aggregate_hits_keys(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                                   const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int top_hits, int order_by,
                                   const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap, const int32_t* q_filter,
                                   const int32_t* q_filter_mask, int32_t* out_groups, int64_t* out_counts, float* out_scores,
                                   int64_t* out_ids, int64_t* out_n_buckets, int64_t* out_total_hits) {
    if (!idx || !out_groups || !out_counts || !out_scores || !out_ids || !out_n_buckets || !out_total_hits)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && (!queries || !min_score))) return fail(RASS_ERR_INVALID, "bad queries / min_score / nq");
    const TopHitsCall a{size, d_keys, n_keys, n_groups, top_hits, order_by, d_allow, n_bitmaps, words_per_bitmap, q_filter,
                        q_filter_mask};
    if (int rc = check_tophits(idx, a, nq)) return rc;
    for (int q = 0; q < nq; ++q)
        if (min_score[q] != min_score[q]) return fail(RASS_ERR_INVALID, "min_score is NaN");
    if (nq == 0) return RASS_OK;
    const TopHitsOut o{out_groups, out_counts, out_scores, out_ids, out_n_buckets, out_total_hits};
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); },
                      [&] { return tophits_once(idx, queries, nq, min_score, a, o); });
}

}  // extern "C"
