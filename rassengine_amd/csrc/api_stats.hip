// api_stats.hip — the C ABI of include/rass_engine.h: the terms aggregation over a key column with a stats sub-aggregation,
// rass_index_aggregate_stats_keys(_device): rass_index_aggregate_keys' buckets, each with the count, sum, min and max of an
// attribute column over its hits, ordered by doc_count or by one of those metrics.  Host-side C++ only: the kernels are
// scan_stats.hip (the one-pass scan into a plane-major table) and group_topk.hip (the select — unchanged for the default
// order — and the gather of the listed buckets' planes).  The table lives in the engine-owned block of the grouped search
// (eng->d_group).  The objects and the threading rules: api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// One launch group (<= 32 queries).  Everything is a device pointer.
struct StatsRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    const float* min_score = nullptr;   // [nq]
    const int32_t* keys = nullptr;      // nullptr: one group
    int64_t n_keys = 0;
    const uint32_t* allow = nullptr;    // this launch group's bitmap(s); allow_q_stride 0: one shared by all of them
    int64_t allow_q_stride = 0, allow_words = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    int32_t* out_groups = nullptr;      // [nq][size]
    int64_t* out_counts = nullptr;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    int64_t* out_vcounts = nullptr;
    int64_t* out_sums = nullptr;
    int32_t* out_mins = nullptr;
    int32_t* out_maxs = nullptr;
    int64_t* n_buckets = nullptr;       // [nq]
    int64_t* total_hits = nullptr;      // [nq]
    int32_t* status = nullptr;          // [1]
};

// What the caller passed, whole.
struct StatsCall {
    int size;
    const int32_t* keys;
    int64_t n_keys;
    int32_t n_groups;
    int value_col, order_by, order_desc;
    const uint32_t* allow;
    int n_bitmaps;
    int64_t words;
    const int32_t* q_filter;
    const int32_t* q_filter_mask;
};

// ... and a launch group's part of it.
void stats_request(StatsRequest& r, const StatsCall& a, int done) {
    r.keys = a.keys, r.n_keys = a.n_keys;
    if (a.allow) {
        r.allow_q_stride = a.n_bitmaps == 1 ? 0 : a.words;
        r.allow = a.allow + (int64_t)done * r.allow_q_stride;
        r.allow_words = a.words;
    }
}

// The argument checks the two entry points share (everything that does not need the row count).
int check_stats(const rass_index* idx, const StatsCall& a, int nq) {
    if (a.size < 1 || a.size > rass::kGroupMaxK) return fail(RASS_ERR_INVALID, "size must be in [1, RASS_MAX_K_MULTIPASS]");
    if (a.n_groups < 1 || a.n_groups > rass::kGroupMaxGroups) return fail(RASS_ERR_INVALID, "n_groups must be in [1, 1048576]");
    if (!a.keys && a.n_groups != 1) return fail(RASS_ERR_INVALID, "d_keys is NULL: the global form needs n_groups == 1");
    if (a.keys && a.n_keys < 0) return fail(RASS_ERR_INVALID, "n_keys is negative");
    if (a.value_col < 0 || a.value_col >= RASS_MAX_ATTRS) return fail(RASS_ERR_INVALID, "value_col must be in [0, RASS_MAX_ATTRS)");
    if (a.order_by != RASS_STATS_BY_COUNT && a.order_by != RASS_STATS_BY_VALUE_COUNT && a.order_by != RASS_STATS_BY_MIN &&
        a.order_by != RASS_STATS_BY_MAX)
        return fail(RASS_ERR_INVALID, "order_by must be one of RASS_STATS_BY_*");
    if (a.q_filter_mask && !a.q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (a.allow) {
        if (a.n_bitmaps != 1 && a.n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
        if (a.words < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    }
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "stats aggregation needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "stats aggregation needs dim <= 1024 (no wide-row form)");
    return RASS_OK;
}

// The table block (eng->d_group, one launch group): the status word, then six planes of [nq][n_groups] — 32 bytes per slot,
// 1 GiB for 32 queries at the n_groups bound.  All adjacent: one memset zeroes everything, and the zeroed table is the empty one.
struct StatsView {
    unsigned* status;              // [1] on a 256-byte line
    unsigned long long* best;
    long long* sum;
    unsigned* count;
    unsigned* vcount;
    unsigned* vmin;
    unsigned* vmax;
    size_t total;
};
StatsView stats_layout(unsigned char* base, int nq, int n_groups) {
    Carver c{base};
    StatsView L;
    const size_t slots = (size_t)nq * n_groups;
    L.status = c.take<unsigned>(sizeof(unsigned));
    L.best = c.take<unsigned long long>(slots * sizeof(unsigned long long));
    L.sum = c.take<long long>(slots * sizeof(long long));
    L.count = c.take<unsigned>(slots * sizeof(unsigned));
    L.vcount = c.take<unsigned>(slots * sizeof(unsigned));
    L.vmin = c.take<unsigned>(slots * sizeof(unsigned));
    L.vmax = c.take<unsigned>(slots * sizeof(unsigned));
    L.total = c.off;
    return L;
}

// normalise -> ONE memset over the status word and every plane -> the stats scan -> the select -> the gather.  Always the exact
// fp32 scan: the prefilter mode of the index is not looked at.  The caller holds eng->mu and has set the device.
int stats_device_group(rass_index* idx, const StatsRequest& r, const StatsCall& a) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const IndexView iv = index_view(idx, /*filtered=*/true, r.id_base);   // tombstones and filters: always read the tags
    if (r.keys && r.n_keys < iv.rows)
        return fail(RASS_ERR_INVALID, "n_keys (" + std::to_string(r.n_keys) + ") is smaller than the index's rows (" + std::to_string(iv.rows) + ")");
    if (r.allow)
        if (int rc = check_words(iv.rows, r.allow_words)) return rc;
    if (iv.rows < 0 || iv.rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (range_layout(nullptr).total > eng->scratch_bytes) return fail(RASS_ERR_INVALID, "scan workspace too small");
    if (int rc = grow_group_table(eng, stats_layout(nullptr, r.nq, a.n_groups).total, st, "stats aggregation")) return rc;
    float* q_padded = range_layout(eng->d_scratch).q_padded;   // where every scan keeps its queries
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, q_padded, idx->stride, r.nq, idx->dim, st, pad_nq(r.nq)));
    const StatsView G = stats_layout(eng->d_group, r.nq, a.n_groups);
    HIP_TRY(hipMemsetAsync(G.status, 0, G.total, st));
    if (iv.rows > 0) {   // an empty index is not scanned: the zeroed table is the answer
        const int grid = scan_grid((iv.rows + 31) / 32, 1, eng->n_cus);
        rass::StatsArgs s;
        s.scan.corpus = iv.corpus;
        s.scan.row_tag = iv.row_tag;
        s.scan.q_padded = q_padded;
        s.scan.q_filter = r.q_filter;
        s.scan.q_filter_mask = r.q_filter_mask;
        s.scan.part_scores = nullptr;
        s.scan.part_ids = nullptr;
        s.scan.row_stride = idx->stride;
        s.scan.id_base = 0;   // the keys name rows of the slab: the select translates them
        s.scan.n_rows = (int)iv.rows;
        s.scan.nq = r.nq;
        s.scan.k = 1;
        s.scan.range_thr = r.min_score;
        s.scan.group_table = G.best;
        s.scan.group_status = G.status;
        s.scan.group_n = a.n_groups;
        s.scan.group_keys = r.keys;
        s.scan.group_key_rows = (int)iv.rows;
        s.scan.allow = r.allow;
        s.scan.allow_q_stride = r.allow_q_stride;
        s.values = idx->d_attr[a.value_col];   // nullptr until the column's first set: reads as all RASS_ATTR_MISSING
        s.count = G.count, s.vcount = G.vcount, s.sum = G.sum, s.vmin = G.vmin, s.vmax = G.vmax;
        const int rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_stats_f32(s, grid, st)); });
        if (rc != RASS_OK) return rc;
    }
    HIP_TRY(rass::launch_group_stats_select(G.count, G.best, G.vcount, G.vmin, G.vmax, a.order_by, a.order_desc != 0, r.nq, a.n_groups,
                                            a.size, iv.id_base, iv.id_map, r.out_groups, r.out_counts, r.out_scores, r.out_ids,
                                            r.n_buckets, r.total_hits, G.status, r.status, st));
    HIP_TRY(rass::launch_group_stats_gather(r.out_groups, G.vcount, G.sum, G.vmin, G.vmax, r.nq, a.n_groups, a.size, r.out_vcounts,
                                            r.out_sums, r.out_mins, r.out_maxs, st));
    return RASS_OK;
}

// The host variant's staging (eng->d_io / the slot's h_io): the aggregation's (AggIoView) with the four stats lists behind it.
struct StatsIoView {
    AggIoView agg;
    int64_t* out_vcounts;          // [32][kGroupMaxK]; a call uses [nq][size]
    int64_t* out_sums;
    int32_t* out_mins;
    int32_t* out_maxs;
    size_t bytes;
};
StatsIoView stats_io_layout(unsigned char* base) {
    StatsIoView L;
    L.agg = agg_io_layout(base);
    Carver c{base, L.agg.bytes};
    const size_t cells = (size_t)RASS_MAX_QBATCH * rass::kGroupMaxK;
    L.out_vcounts = c.take<int64_t>(cells * sizeof(int64_t));
    L.out_sums = c.take<int64_t>(cells * sizeof(int64_t));
    L.out_mins = c.take<int32_t>(cells * sizeof(int32_t));
    L.out_maxs = c.take<int32_t>(cells * sizeof(int32_t));
    L.bytes = c.off;
    return L;
}

// What the host variant writes.
struct StatsOut {
    int32_t* groups;
    int64_t* counts;
    float* scores;
    int64_t* ids;
    int64_t* vcounts;
    int64_t* sums;
    int32_t* mins;
    int32_t* maxs;
    int64_t* n_buckets;
    int64_t* total_hits;
};

// One attempt of the host call.  A group whose scan met a hit with a key >= n_groups ends the call.
int stats_once(rass_index* idx, const float* queries, int nq, const float* min_score, const StatsCall& a, const StatsOut& o) {
    rass_engine* eng = idx->eng;
    const int size = a.size;
    return host_groups(
        idx, queries, nq, a.q_filter, a.q_filter_mask, stats_io_layout(nullptr).bytes,
        [&](HostSlot* sl, int done, int b) {
            memcpy(stats_io_layout(static_cast<unsigned char*>(sl->h_io)).agg.thr, min_score + done, (size_t)b * sizeof(float));
        },
        [&](HostSlot* sl, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const StatsIoView H = stats_io_layout(static_cast<unsigned char*>(sl->h_io)), D = stats_io_layout(eng->d_io);
            const size_t cells = (size_t)b * size;
            HIP_TRY(hipMemcpyAsync(D.agg.thr, H.agg.thr, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            StatsRequest r;
            stats_request(r, a, done);
            r.queries = eng->d_qraw, r.nq = b, r.min_score = D.agg.thr;
            r.q_filter = a.q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = a.q_filter_mask ? eng->d_qmask : nullptr;
            r.out_groups = D.agg.out_groups, r.out_counts = D.agg.out_counts, r.out_scores = D.agg.out_scores, r.out_ids = D.agg.out_ids;
            r.out_vcounts = D.out_vcounts, r.out_sums = D.out_sums, r.out_mins = D.out_mins, r.out_maxs = D.out_maxs;
            r.n_buckets = D.agg.n_buckets, r.total_hits = D.agg.total_hits, r.status = D.agg.status;
            if (int grc = stats_device_group(idx, r, a)) return grc;
            HIP_TRY(hipMemcpyAsync(H.agg.n_buckets, D.agg.n_buckets, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.agg.total_hits, D.agg.total_hits, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.agg.status, D.agg.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.agg.out_groups, D.agg.out_groups, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.agg.out_counts, D.agg.out_counts, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.agg.out_scores, D.agg.out_scores, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.agg.out_ids, D.agg.out_ids, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_vcounts, D.out_vcounts, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_sums, D.out_sums, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_mins, D.out_mins, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_maxs, D.out_maxs, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            const StatsIoView H = stats_io_layout(static_cast<unsigned char*>(sl->h_io));
            const size_t cells = (size_t)b * size;
            const int64_t at = (int64_t)done * size;
            if (*H.agg.status != 0)
                return fail(RASS_ERR_INVALID, "stats aggregation: a hit's group key is >= n_groups (" + std::to_string(a.n_groups) + ")");
            memcpy(o.n_buckets + done, H.agg.n_buckets, (size_t)b * sizeof(int64_t));
            memcpy(o.total_hits + done, H.agg.total_hits, (size_t)b * sizeof(int64_t));
            memcpy(o.groups + at, H.agg.out_groups, cells * sizeof(int32_t));
            memcpy(o.counts + at, H.agg.out_counts, cells * sizeof(int64_t));
            memcpy(o.scores + at, H.agg.out_scores, cells * sizeof(float));
            memcpy(o.ids + at, H.agg.out_ids, cells * sizeof(int64_t));
            memcpy(o.vcounts + at, H.out_vcounts, cells * sizeof(int64_t));
            memcpy(o.sums + at, H.out_sums, cells * sizeof(int64_t));
            memcpy(o.mins + at, H.out_mins, cells * sizeof(int32_t));
            memcpy(o.maxs + at, H.out_maxs, cells * sizeof(int32_t));
            return RASS_OK;
        });
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_aggregate_stats_keys_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                           const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int value_col, int order_by,
                                           int order_desc, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                           const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base,
                                           int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores, int64_t* d_out_ids,
                                           int64_t* d_out_value_counts, int64_t* d_out_sums, int32_t* d_out_mins, int32_t* d_out_maxs,
                                           int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status) {
    if (!idx || !d_queries || !d_min_score || !d_out_groups || !d_out_counts || !d_out_scores || !d_out_ids || !d_out_value_counts ||
        !d_out_sums || !d_out_mins || !d_out_maxs || !d_n_buckets || !d_total_hits || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    const StatsCall a{size, d_keys, n_keys, n_groups, value_col, order_by, order_desc, d_allow, n_bitmaps, words_per_bitmap,
                      d_q_filter, d_q_filter_mask};
    if (int rc = check_stats(idx, a, nq)) return rc;
    StatsRequest r;
    stats_request(r, a, 0);
    r.queries = d_queries, r.nq = nq, r.min_score = d_min_score;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_groups = d_out_groups, r.out_counts = d_out_counts, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    r.out_vcounts = d_out_value_counts, r.out_sums = d_out_sums, r.out_mins = d_out_mins, r.out_maxs = d_out_maxs;
    r.n_buckets = d_n_buckets, r.total_hits = d_total_hits, r.status = d_status;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    const int rc = set_device(eng);
    return rc != RASS_OK ? rc : stats_device_group(idx, r, a);
}

int rass_index_aggregate_stats_keys(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                                    const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int value_col, int order_by,
                                    int order_desc, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                    const int32_t* q_filter, const int32_t* q_filter_mask, int32_t* out_groups, int64_t* out_counts,
                                    float* out_scores, int64_t* out_ids, int64_t* out_value_counts, int64_t* out_sums,
                                    int32_t* out_mins, int32_t* out_maxs, int64_t* out_n_buckets, int64_t* out_total_hits) {
    if (!idx || !out_groups || !out_counts || !out_scores || !out_ids || !out_value_counts || !out_sums || !out_mins || !out_maxs ||
        !out_n_buckets || !out_total_hits)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && (!queries || !min_score))) return fail(RASS_ERR_INVALID, "bad queries / min_score / nq");
    const StatsCall a{size, d_keys, n_keys, n_groups, value_col, order_by, order_desc, d_allow, n_bitmaps, words_per_bitmap,
                      q_filter, q_filter_mask};
    if (int rc = check_stats(idx, a, nq)) return rc;
    for (int q = 0; q < nq; ++q)
        if (min_score[q] != min_score[q]) return fail(RASS_ERR_INVALID, "min_score is NaN");
    if (nq == 0) return RASS_OK;
    const StatsOut o{out_groups, out_counts, out_scores, out_ids, out_value_counts, out_sums, out_mins, out_maxs, out_n_buckets,
                     out_total_hits};
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); },
                      [&] { return stats_once(idx, queries, nq, min_score, a, o); });
}

}  // extern "C"
